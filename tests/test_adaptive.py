"""Per-tile adaptive sampling on the GPU (include/fountain_hip_adaptive.h, fountain_amd/adaptive.py): with n0 = N it is one moments
render; with a huge threshold every tile stops at n0; a mixed schedule equals, tile by tile, uniform moments renders over [0, n) at each
tile's count, and that schedule is the one the host twin of the criterion gives on those uniform buffers; black tiles stop at n0 and the
statistics agree with the counts; host and device entries; quality at equal samples; several chunks per round; refusals; the CLI.

Every uniform reference keeps samples_per_pixel = N and renders the sample range [0, n) (camera_ray_diff scales by 1/sqrt(N))."""
import ctypes as C
import os

import numpy as np
import pytest

from fountain_amd import (DirectLightingIntegrator, FountainError, PathIntegrator, PerspectiveCamera, RandomSampler, SceneBuilder,
                          WhittedIntegrator, scenes, _abi as A)
from fountain_amd import adaptive as AD
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


def sphere_on_black(be, res=64):
    """a matte sphere on a floor, lit by a small spherical emitter, under a black sky: the top of the image is black, the floor and the
    sphere's shadowed side are noisy"""
    b = SceneBuilder(be)
    b.attribute_begin(); b.material("matte", Kd=(0.0, 0.0, 0.0)); b.area_light_source("diffuse", L=(30.0, 30.0, 30.0))
    b.translate((1.6, 0.5, 2.2)); b.shape("sphere", radius=0.25); b.attribute_end()
    b.attribute_begin(); b.material("matte", Kd=(0.7, 0.55, 0.4)); b.translate((-0.4, 0.0, 0.0)); b.shape("sphere", radius=0.8); b.attribute_end()
    b.attribute_begin(); b.material("matte", Kd=(0.5, 0.5, 0.5))
    scenes._quad(b, (-6, -6, -0.8), (6, -6, -0.8), (6, 6, -0.8), (-6, 6, -0.8)); b.attribute_end()
    cam = PerspectiveCamera.look_at(be, (0.0, -5.0, 0.3), (0.0, 0.0, 0.3), (0, 0, 1), (res, res), fov=50.0)
    return b, cam, (res, res)


def uniform(be, scene, cam, res, integ, N, n, seed, crop=(0.0, 0.0, 1.0, 1.0), radius=(0.5, 0.5), tiles=None):
    """ftn_render_moments with samples_per_pixel = N over the sample range [0, n): (pixels, moments, stats)"""
    _, film, mom, st = M.render_moments(be, None, cam, res, integ, RandomSampler(N, seed, indexed=True, first_sample=0, sample_count=n),
                                        scene=scene, film=GR.film(be, res, crop, radius), tiles=tiles)
    return film.pixels, mom, st


def adaptive(be, scene, cam, res, integ, N, seed, prm, crop=(0.0, 0.0, 1.0, 1.0), radius=(0.5, 0.5), tiles=None):
    film, mom, cnt, info, st = AD.render_adaptive(be, None, cam, res, integ, RandomSampler(N, seed, indexed=True), prm, scene=scene,
                                                  film=GR.film(be, res, crop, radius), tiles=tiles)
    return film.pixels, mom, cnt, info, st


def schedule(n0, N, step):
    s = [n0]
    while s[-1] < N:
        s.append(min(N, s[-1] + (step or s[-1])))
    return s


def tile_of(film_like, res, crop=(0.0, 0.0, 1.0, 1.0), radius=(0.5, 0.5), tiles=None):
    """per crop pixel, the index of its tile in the tile range (-1 outside), and the tiles' crop-pixel slices"""
    f = GR.film(film_like, res, crop, radius)
    c = f.desc.crop
    sel = GR.selected_tiles(f, tiles)
    idx = np.full((f.height, f.width), -1, np.int64)
    sl = []
    for k, (x0, y0, x1, y1) in enumerate(sel):
        ys = slice(max(y0, c[1]) - c[1], max(min(y1, c[3]) - c[1], 0))
        xs = slice(max(x0, c[0]) - c[0], max(min(x1, c[2]) - c[0], 0))
        idx[ys, xs] = k
        sl.append((ys, xs))
    return idx, sl


def check_equal(got, want, own, what):
    """bit-equal where no foreign sample landed (own), the moments tests' tolerance elsewhere; weights bit-equal everywhere"""
    assert np.array_equal(bits(got[own]), bits(want[own])), what
    assert np.allclose(got, want, rtol=1e-5, atol=1e-6), what


# ------------------------------------------------------------------ 1. n0 = N: one round, ftn_render_moments
CASES = [("cornell", "path", (0.5, 0.5), (0.0, 0.0, 1.0, 1.0), None),
         ("cornell", "path", (1.25, 1.25), (0.1, 0.05, 0.9, 0.95), (1, 2, 0)),
         ("cornell", "direct", (0.5, 0.5), (0.0, 0.0, 1.0, 1.0), (0, 2, 0)),
         ("cornell", "whitted", (1.25, 1.25), (0.0, 0.0, 1.0, 1.0), None),
         ("black", "path", (0.5, 0.5), (0.2, 0.0, 1.0, 0.8), None)]


@pytest.mark.parametrize("which,integ,radius,crop,tiles", CASES)
def test_one_round_is_render_moments(gpu, which, integ, radius, crop, tiles):
    N, seed = 6, 23
    b, cam, res = scenes.cornell(gpu, res=40) if which == "cornell" else sphere_on_black(gpu, 40)
    integrator = {"path": PathIntegrator(5, 1.0), "direct": DirectLightingIntegrator(4), "whitted": WhittedIntegrator(4)}[integ]
    scene = b.create_scene()
    want, m_want, st_want = uniform(gpu, scene, cam, res, integrator, N, N, seed, crop, radius, tiles)
    got, m_got, cnt, info, st = adaptive(gpu, scene, cam, res, integrator, N, seed, AD.params(gpu, min_samples=N), crop, radius, tiles)
    assert counters(st) == counters(st_want)
    assert info["rounds"] == 1 and info["tiles_at_max"] == info["tiles"] == len(GR.selected_tiles(GR.film(gpu, res, crop, radius), tiles))
    idx, _ = tile_of(gpu, res, crop, radius, tiles)
    assert (cnt[idx >= 0] == N).all() and (cnt[idx < 0] == 0).all()
    assert info["pixel_samples"] == N * int((idx >= 0).sum())
    assert np.array_equal(bits(got[..., 3]), bits(want[..., 3]))
    own = want[..., 3] == (N if radius[0] == 0.5 else -1)
    check_equal(got, want, own, "beauty")
    check_equal(m_got, m_want, own, "moments")


# ------------------------------------------------------------------ 1b. decisions with spill and a crop
SPILL_CASES = [((1.25, 1.25), (0.1, 0.05, 0.9, 0.95), None),
               ((1.5, 0.75), (0.0, 0.1, 0.85, 1.0), (1, 2, 0))]


@pytest.mark.parametrize("radius,crop,tiles", SPILL_CASES)
def test_decisions_with_spill_and_crop(gpu, radius, crop, tiles):
    """n0 = 4, N = 16, doubling: decisions after 4 and after 8 samples, on sums with in-tile and other-tile spill, in a crop that cuts
    through tiles.  A tile stops at n iff the host twin passes every one of its crop pixels on a uniform [0, n) moments render of the
    same film (and failed at the count before).  The threshold lies between two tiles' requirements at n0; a tile is left out only where
    the twin's verdict changes when t moves by 0.1 % (the spill sums come from atomics, so their last bits can differ between renders)."""
    n0, N, seed, a = 4, 16, 31, 0.01
    b, cam, res = scenes.cornell(gpu, res=96)
    scene = b.create_scene()
    integ = PathIntegrator(5, 1.0)
    u = {n: uniform(gpu, scene, cam, res, integ, N, n, seed, crop, radius, tiles) for n in (n0, 2 * n0)}
    assert u[n0][2]["spill_samples"] > 1000                             # the spilled branch: in-tile and other-tile sums
    idx, sl = tile_of(gpu, res, crop, radius, tiles)
    live = [k for k, (ys, xs) in enumerate(sl) if idx[ys, xs].size]

    def verdicts(n, t):
        conv = AD.converged(gpu, u[n][0], u[n][1], AD.params(gpu, min_samples=n0, threshold=t, abs_floor=a)).astype(bool)
        return np.array([conv[sl[k]].all() for k in live])
    # each tile's smallest passing t at n0 (bisection on the host twin), then a threshold between two neighbouring tiles
    need = []
    for k in live:
        lo, hi = 0.0, 1e3
        for _ in range(40):
            mid = (lo + hi) / 2
            ok = AD.converged(gpu, u[n0][0][sl[k]], u[n0][1][sl[k]], AD.params(gpu, min_samples=n0, threshold=mid, abs_floor=a)).all()
            lo, hi = (lo, mid) if ok else (mid, hi)
        need.append(hi)
    srt = sorted(need)
    h = len(srt) // 2
    t = float(np.sqrt(srt[h - 1] * srt[h]))
    v = {n: (verdicts(n, t * (1 - 1e-3)), verdicts(n, t), verdicts(n, t * (1 + 1e-3))) for n in (n0, 2 * n0)}
    sure = {n: v[n][0] == v[n][2] for n in v}
    pass1, pass2 = v[n0][1], v[2 * n0][1]
    assert sure[n0].sum() >= len(live) - 2 and pass1[sure[n0]].sum() >= 3 and (~pass1[sure[n0]]).sum() >= 3
    stop2 = sure[n0] & sure[2 * n0] & ~pass1 & pass2                    # tiles that must stop after the second round
    assert stop2.sum() >= 1
    prm = AD.params(gpu, min_samples=n0, threshold=t, abs_floor=a)
    got, m_got, cnt, info, st = adaptive(gpu, scene, cam, res, integ, N, seed, prm, crop, radius, tiles)
    assert info["rounds"] == (3 if info["tiles_at_max"] else 2) and st["spill_samples"] > 1000
    for j, k in enumerate(live):
        c = cnt[sl[k]]
        assert (c == c.flat[0]).all() and c.flat[0] in (n0, 2 * n0, N), (k, c.flat[0])
        if sure[n0][j]:
            assert (c.flat[0] == n0) == pass1[j], (k, need[j], t)
        if sure[n0][j] and sure[2 * n0][j] and not pass1[j]:
            assert (c.flat[0] == 2 * n0) == pass2[j], (k, t)
    # tiles without a crop pixel (edge tiles of the sample bounds) converge after round 1: only live tiles can reach N
    at_max = ~pass1 & ~pass2
    unsure = int((~(sure[n0] & sure[2 * n0])).sum())
    assert int(at_max.sum()) - unsure <= info["tiles_at_max"] <= int(at_max.sum()) + unsure
    assert info["tiles"] == len(sl) and (cnt[idx < 0] == 0).all()


# ------------------------------------------------------------------ 2. a huge threshold: every tile stops at n0
def test_huge_threshold_stops_at_n0(gpu):
    N, n0, seed = 32, 4, 5
    b, cam, res = sphere_on_black(gpu, 48)
    scene = b.create_scene()
    integ = PathIntegrator(5, 1.0)
    got, m_got, cnt, info, st = adaptive(gpu, scene, cam, res, integ, N, seed, AD.params(gpu, min_samples=n0, threshold=1e15, abs_floor=1.0))
    want, m_want, st_want = uniform(gpu, scene, cam, res, integ, N, n0, seed)
    assert info["rounds"] == 1 and info["tiles_at_max"] == 0 and (cnt == n0).all()
    assert counters(st) == counters(st_want) and st["camera_samples"] == n0 * res[0] * res[1] == info["pixel_samples"]
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(m_got), bits(m_want))


# ------------------------------------------------------------------ 3./4. mixed schedules, tile by tile, and the schedule itself
@pytest.mark.parametrize("step", [0, 12])
def test_mixed_schedule(gpu, step):
    N, n0, seed, t, a = 64, 8, 3, 0.05, 0.01
    b, cam, res = sphere_on_black(gpu, 64)
    scene = b.create_scene()
    integ = PathIntegrator(5, 1.0)
    prm = AD.params(gpu, min_samples=n0, step_samples=step, threshold=t, abs_floor=a)
    got, m_got, cnt, info, st = adaptive(gpu, scene, cam, res, integ, N, seed, prm)
    sched = schedule(n0, N, step)
    idx, sl = tile_of(gpu, res)
    tile_n = np.array([int(cnt[ys, xs].flat[0]) for ys, xs in sl])
    for k, (ys, xs) in enumerate(sl):
        assert (cnt[ys, xs] == tile_n[k]).all()
    assert set(tile_n) <= set(sched) and len(set(tile_n)) >= 2, sorted(tile_n)
    assert info["rounds"] == sched.index(max(tile_n)) + 1 and info["tiles_at_max"] == int((tile_n == N).sum())
    # 4. the black sky stops at n0, and the statistics follow the counts
    black = [k for k, (ys, xs) in enumerate(sl) if not got[ys, xs, :3].any()]
    assert len(black) >= 4 and (tile_n[black] == n0).all()
    assert st["camera_samples"] == int(cnt.sum()) == info["pixel_samples"] < N * cnt.size
    assert st["spill_samples"] <= 4                                    # radius 0.5: only samples on a pixel edge land elsewhere
    print("step %d: tiles per count %s, %.1f samples per pixel" % (step, {n: int((tile_n == n).sum()) for n in sched}, cnt.mean()))
    # 3. per count, a uniform moments render over [0, n) holds the same bits; the host twin gives the schedule on those buffers
    uni = {}
    for n in sched:
        if n in tile_n or any(sched[i + 1] in tile_n for i in range(len(sched) - 1) if sched[i] == n):
            uni[n] = uniform(gpu, scene, cam, res, integ, N, n, seed)
    # a pixel reached by a sample of another pixel (weight other than its count, here or in the uniform render) mixes two counts when
    # the tiles differ: it is left out of the bit comparison, and its tile out of the schedule check
    foreign = (got[..., 3] != cnt) | (uni[n0][0][..., 3] != n0)
    assert foreign.sum() <= 2 * st["spill_samples"] + 2 * uni[n0][2]["spill_samples"]
    for k, (ys, xs) in enumerate(sl):
        n = int(tile_n[k])
        u_px, u_m, _ = uni[n]
        own = ~foreign[ys, xs] & (u_px[ys, xs, 3] == n)
        assert np.array_equal(bits(got[ys, xs][own]), bits(u_px[ys, xs][own])), (k, n)
        assert np.array_equal(bits(m_got[ys, xs][own]), bits(u_m[ys, xs][own])), (k, n)
        if not own.all():
            continue
        if n < N:
            assert AD.converged(gpu, u_px[ys, xs], u_m[ys, xs], prm).all(), (k, n)
        if n > n0:
            p_px, p_m, _ = uni[sched[sched.index(n) - 1]]
            assert not AD.converged(gpu, p_px[ys, xs], p_m[ys, xs], prm).all(), (k, n)


# ------------------------------------------------------------------ 5. host and device entries
def test_host_and_device_entries(gpu):
    import torch
    N, n0, seed = 32, 4, 9
    b, cam, res = sphere_on_black(gpu, 48)
    scene = b.create_scene()
    integ = PathIntegrator(5, 1.0)
    prm = AD.params(gpu, min_samples=n0, threshold=0.1)
    tiles = (1, 2, 0)
    px0, m0, cnt0, info0, st0 = adaptive(gpu, scene, cam, res, integ, N, seed, prm, tiles=tiles)
    idx, _ = tile_of(gpu, res, tiles=tiles)
    assert (cnt0[idx < 0] == 0).all() and (cnt0[idx >= 0] >= n0).all() and len(np.unique(cnt0[idx >= 0])) >= 2
    # the host entry adds into non-zero caller buffers and leaves counts outside the tile range alone
    rng = np.random.default_rng(2)
    e_px, e_m = rng.uniform(0, 3, px0.shape).astype(F32), rng.uniform(0, 3, m0.shape).astype(F32)
    film = GR.film(gpu, res)
    film.pixels[...] = e_px
    sentinel = np.full(cnt0.shape, 12345, np.uint32)
    film, m_h, cnt_h, info_h, st_h = AD.render_adaptive(gpu, None, cam, res, integ, RandomSampler(N, seed, indexed=True), prm, scene=scene,
                                                        film=film, moments=e_m.copy(), counts=sentinel, tiles=tiles)
    assert np.array_equal(bits(film.pixels), bits((e_px + px0).astype(F32))) and np.array_equal(bits(m_h), bits((e_m + m0).astype(F32)))
    assert (cnt_h[idx < 0] == 12345).all() and np.array_equal(cnt_h[idx >= 0], cnt0[idx >= 0])
    assert info_h == info0 and counters(st_h) == counters(st0)
    # the device entry: the same bits from zero tensors, counts written only for the tile range
    t_px = torch.zeros(px0.shape, dtype=torch.float32, device="cuda")
    t_m = torch.zeros_like(t_px)
    t_n = torch.full(cnt0.shape, -7, dtype=torch.int32, device="cuda")
    info_d, st_d = AD.render_adaptive_torch(scene, cam, GR.film(gpu, res), integ, RandomSampler(N, seed, indexed=True), prm, t_px, t_m, t_n, tiles=tiles)
    torch.cuda.synchronize()
    d_n = t_n.cpu().numpy()
    assert np.array_equal(bits(t_px.cpu().numpy()), bits(px0)) and np.array_equal(bits(t_m.cpu().numpy()), bits(m0))
    assert (d_n[idx < 0] == -7).all() and np.array_equal(d_n[idx >= 0].astype(np.uint32), cnt0[idx >= 0])
    assert info_d == info0 and counters(st_d) == counters(st0)
    # and on a stream of its own
    s = torch.cuda.Stream()
    t_px.zero_(); t_m.zero_(); torch.cuda.synchronize()
    AD.render_adaptive_torch(scene, cam, GR.film(gpu, res), integ, RandomSampler(N, seed, indexed=True), prm, t_px, t_m, t_n, tiles=tiles, stream=s)
    s.synchronize()
    assert np.array_equal(bits(t_px.cpu().numpy()), bits(px0))


# ------------------------------------------------------------------ 6. quality at equal samples
def test_quality_against_uniform_at_equal_samples(gpu):
    N, seed = 64, 4
    b, cam, res = sphere_on_black(gpu, 64)
    scene = b.create_scene()
    integ = PathIntegrator(5, 1.0)
    ref, _, _ = uniform(gpu, scene, cam, res, integ, 1024, 1024, 1000)
    got, _, cnt, info, st = adaptive(gpu, scene, cam, res, integ, N, seed, AD.params(gpu))
    spp = -(-int(st["camera_samples"]) // cnt.size)                     # a uniform render with at least as many camera samples
    assert spp < N
    uni, _, st_u = uniform(gpu, scene, cam, res, integ, spp, spp, seed)
    assert st_u["camera_samples"] >= st["camera_samples"]

    def rgb(p):
        """the film's resolve (ftn_film_resolve): xyz_to_rgb(xyz) / W, clamped at 0"""
        out = np.zeros(p.shape[:-1] + (3,), F32)
        gpu.lib.ftn_film_resolve(np.ascontiguousarray(p, F32).ctypes.data_as(C.c_void_p), C.c_size_t(p.size // 4), out.ctypes.data_as(C.c_void_p))
        return out.astype(np.float64)

    def rel_mse(p):
        r = rgb(ref)
        return float((((rgb(p) - r) ** 2) / (r * r + 1e-2)).mean())
    e_a, e_u = rel_mse(got), rel_mse(uni)
    print("relative MSE: adaptive %.3g (%.1f spp), uniform %.3g (%d spp)" % (e_a, cnt.mean(), e_u, spp))
    assert e_a < 0.8 * e_u


# ------------------------------------------------------------------ 7. several chunks per round
def test_multi_chunk_rounds(gpu, monkeypatch):
    N, n0, seed = 32, 4, 12
    b, cam, res = sphere_on_black(gpu, 512)
    scene = b.create_scene()
    integ = PathIntegrator(3, 1.0)
    prm = AD.params(gpu, min_samples=n0, threshold=0.1)
    one = adaptive(gpu, scene, cam, res, integ, N, seed, prm)
    monkeypatch.setenv("FTN_WF_PATHS_M", "1")                          # 2^20 paths per chunk: 4 samples of 1024 tiles
    many = adaptive(gpu, scene, cam, res, integ, N, seed, prm)
    monkeypatch.delenv("FTN_WF_PATHS_M")
    assert many[4]["trace_launches"] > one[4]["trace_launches"]
    work = lambda st: {k: v for k, v in counters(st).items() if not k.endswith("_launches")}
    assert work(many[4]) == work(one[4]) and many[3] == one[3] and one[3]["rounds"] >= 3
    for k in range(3):
        assert np.array_equal(bits(many[k]) if k < 2 else many[k], bits(one[k]) if k < 2 else one[k]), k


# ------------------------------------------------------------------ refusals and errors
def test_refusals_and_nan(gpu):
    b, cam, res = scenes.cornell(gpu, res=16)
    scene = b.create_scene()
    integ = PathIntegrator(3, 1.0)
    prm = AD.params(gpu, min_samples=2)
    for smp, pl, code in ((RandomSampler(4, 0), AUTO, A.FTN_ERR_UNSUPPORTED), (RandomSampler(4, 0, indexed=True), MEGA, A.FTN_ERR_UNSUPPORTED),
                          (RandomSampler(4, 0, indexed=True, first_sample=1, sample_count=3), AUTO, A.FTN_ERR_INVALID_ARGUMENT)):
        with pytest.raises(FountainError) as e:
            AD.render_adaptive(gpu, None, cam, res, integ, smp, prm, scene=scene, pipeline=pl)
        assert e.value.code == code

    def many_lights(be, n):
        bb, c, r = scenes.cornell(be, res=16)
        for k in range(n):
            bb.light_source("point", I=(1 + 0.1 * k, 1, 1), from_=(0.07 * k - 0.5, 0.03 * k, 0.5))
        return bb, c, r
    n_area = len(many_lights(gpu, 0)[0].create_scene().lights()[0])
    bb, c, r = many_lights(gpu, 33 - n_area)
    with pytest.raises(FountainError) as e:
        AD.render_adaptive(gpu, bb, c, r, WhittedIntegrator(3), RandomSampler(4, 0, indexed=True), prm)
    assert e.value.code == A.FTN_ERR_UNSUPPORTED
    # NaN radiance stops the schedule after its round; the buffers are still written and the code returned
    nb, ncam, nres = scenes.cornell(gpu, res=16)
    nb.attribute_begin(); nb.material("matte", Kd=(0.0, 0.0, 0.0)); nb.area_light_source("diffuse", L=(float("nan"), 1.0, 1.0))
    scenes._quad(nb, (-0.2, 0.99, -0.2), (0.2, 0.99, -0.2), (0.2, 0.99, 0.2), (-0.2, 0.99, 0.2)); nb.attribute_end()
    nscene = nb.create_scene()
    film = GR.film(gpu, nres)
    mom, cnt = np.zeros((16, 16, 4), F32), np.zeros((16, 16), np.uint32)
    args, keep = M._call_args(ncam, film, integ, RandomSampler(16, 0, indexed=True), None, AUTO, -1)
    info, st = A.ftn_adaptive_info(), A.ftn_stats()
    rc = gpu.lib.ftn_render_adaptive(nscene.handle, *args, C.byref(AD.params(gpu, min_samples=2, threshold=0.0)), film.pixels.ctypes.data_as(C.c_void_p),
                                     mom.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), C.byref(info), C.byref(st))
    assert rc == A.FTN_ERR_NAN_RADIANCE
    assert info.rounds == 1 and (cnt == 2).all() and (film.pixels[..., 3] == 2).all()


# ------------------------------------------------------------------ 8. the CLI
def test_cli_writes_the_counts(gpu, tmp_path):
    from fountain_amd import render
    from fountain_amd.api import PbrtScene, read_exr
    scene_file = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")
    plain, ad = str(tmp_path / "plain.exr"), str(tmp_path / "ad.exr")
    assert render.main([scene_file, "-o", plain, "--samples", "8"]) == 0
    assert render.main([scene_file, "-o", ad, "--samples", "16", "--adaptive", "0.2", "--min-samples", "4", "--variance"]) == 0
    parsed = PbrtScene(scene_file, gpu)
    film, mom, cnt, info, st = AD.render_adaptive(gpu, None, parsed.camera, None, PathIntegrator(5, 1.0), parsed.sampler(16, indexed=True),
                                                  AD.params(gpu, min_samples=4, threshold=0.2), scene=parsed.create_scene(), film=parsed.film())
    img, _ = film.into_spectrum_buffer()
    assert np.array_equal(bits(read_exr(ad, gpu)), bits(np.asarray(img).reshape(read_exr(ad, gpu).shape)))
    spp = read_exr(render.spp_path(ad), gpu)
    assert np.array_equal(spp, np.repeat(cnt.astype(F32)[..., None], 3, -1)) and set(np.unique(cnt)) <= {4, 8, 16}
    assert np.array_equal(bits(read_exr(render.variance_path(ad), gpu)), bits(M.resolve(gpu, film.pixels, mom)[..., :3]))
    assert not os.path.exists(render.spp_path(plain))
    # fewer samples than the default min_samples: n0 becomes the samples per pixel, one round
    small = str(tmp_path / "small.exr")
    assert render.main([scene_file, "-o", small, "--samples", "4", "--adaptive", "0.05"]) == 0
    assert (read_exr(render.spp_path(small), gpu) == 4).all()
    for extra in (["--exact-stream"], ["--gbuffer"], ["--denoise"], ["--gpus", "2"]):
        assert render.main([scene_file, "-o", str(tmp_path / "x.exr"), "--adaptive", "0.1"] + extra) == 2, extra
