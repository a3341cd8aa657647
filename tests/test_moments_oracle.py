"""The moments (include/fountain_hip_moments.h) and adaptive sampling (include/fountain_hip_adaptive.h) on the GPU against the CPU oracle's
radiance of every camera sample (_moments_ref.py): weights bit-equal everywhere; the beauty and all four moment sums bit-equal wherever
no sample of another pixel landed and within the reordering bound elsewhere; the sample statistics; chunked passes whose film positions
decide the footprints; the variance resolve against float64; the adaptive schedule against the simulator, and its mixed-count image
against the reference built from the GPU's own counts."""
import numpy as np
import pytest

from fountain_amd import DirectLightingIntegrator, PathIntegrator, PerspectiveCamera, RandomSampler, WhittedIntegrator, scenes
from fountain_amd import adaptive as AD
from fountain_amd import moments as M

import _gbuffer_ref as GR
import _moments_ref as MR
from test_adaptive import sphere_on_black
from test_moments import textured_env
from test_moments_cpu import constant_sphere

pytestmark = pytest.mark.gpu
F32 = np.float32
INTEGRATORS = {"path": lambda: PathIntegrator(5, 1.0), "direct": lambda: DirectLightingIntegrator(4), "whitted": lambda: WhittedIntegrator(4),
               "path1": lambda: PathIntegrator(1, 1.0), "path3": lambda: PathIntegrator(3, 1.0)}
FULL = (0.0, 0.0, 1.0, 1.0)
R05, R125, R1575 = (0.5, 0.5), (1.25, 1.25), (1.5, 0.75)
CROP = (0.1, 0.05, 0.9, 0.95)


def cubes(be):
    """a small thin-lens instanced_cubes with a checkerboard: defocus blur, textures under lens-shifted differentials"""
    return scenes.instanced_cubes(be, n_copies=8, res=(48, 40), env_n=64, lens_radius=3.0, textured=True)


def slit(be):
    """sphere_on_black through a 12992 x 2 film (a narrow field of view, 813 tiles at radius 1.25): with FTN_WF_PATHS_M=1 a pass holds
    2^20 / (813 * 256) = 5 samples, at 52k camera samples per sample index"""
    b, _, _ = sphere_on_black(be, 16)
    res = (12992, 2)
    cam = PerspectiveCamera.look_at(be, (0.0, -5.0, 0.3), (0.0, 0.0, -0.5), (0, 0, 1), res, fov=0.018)
    return b, cam, res


SCENES = {"cornell": lambda be: scenes.cornell(be, res=40), "floor": lambda be: GR.textured_floor(be),
          "floor_solid": lambda be: GR.textured_floor(be, null_layer=False), "env": textured_env, "cubes": cubes,
          "row": lambda be: scenes.cornell(be, res=40)[:2] + ((37, 1),), "col": lambda be: scenes.cornell(be, res=40)[:2] + ((1, 37),),
          "odd": lambda be: scenes.cornell(be, res=40)[:2] + ((17, 33),), "black": lambda be: sphere_on_black(be, 64),
          "black96": lambda be: sphere_on_black(be, 96), "slit": slit}


def _camera(be, which):
    """scenes whose camera has its own resolution: rebuild the camera for the film's"""
    b, cam, res = SCENES[which](be)
    if which in ("row", "col", "odd"):
        cam = PerspectiveCamera.look_at(be, (0.0, -3.4, 0.0), (0.0, 0.0, 0.0), (0, 0, 1), res, fov=40.0)
    return b, cam, res


# ------------------------------------------------------------------ 1. moments against the records
MOMENT_CASES = [
    ("cornell", "path", R05, FULL, None, 4, 0, 0), ("cornell", "direct", R05, FULL, None, 4, 0, 0), ("cornell", "whitted", R05, FULL, None, 4, 0, 0),
    ("cornell", "path", R125, CROP, None, 20, 3, 13), ("cornell", "direct", R125, CROP, None, 20, 3, 13),
    ("cornell", "whitted", R1575, (0.0, 0.1, 0.85, 1.0), (1, 2, 0), 20, 3, 13),
    ("floor", "path", R05, FULL, None, 8, 0, 0), ("floor_solid", "direct", R125, CROP, None, 8, 0, 0),
    ("floor_solid", "whitted", R1575, FULL, (1, 2, 0), 20, 3, 13), ("floor_solid", "direct", R05, FULL, None, 20, 3, 13),
    ("env", "path", R125, CROP, None, 6, 0, 0), ("env", "direct", R05, FULL, (0, 2, 0), 20, 3, 13),
    ("cubes", "path", R05, FULL, None, 4, 0, 0), ("cubes", "path", R125, FULL, None, 20, 3, 13),
    ("row", "path", R125, FULL, None, 8, 0, 0), ("col", "direct", R1575, FULL, None, 8, 0, 0), ("odd", "whitted", R125, FULL, (1, 2, 0), 20, 3, 13),
]


def _moments_case(gpu, orc_det, which, integ, radius, crop, tiles, spp, first, count, seed=17):
    smp = RandomSampler(spp, seed, indexed=True, first_sample=first, sample_count=count)
    b, cam, res = _camera(gpu, which)
    _, film, mom, st = M.render_moments(gpu, None, cam, res, INTEGRATORS[integ](), smp, tiles=tiles, scene=b.create_scene(),
                                        film=GR.film(gpu, res, crop, radius))
    rec, f, _ = MR.oracle_records(orc_det, lambda be: _camera(be, which), INTEGRATORS[integ](), smp, crop, radius, tiles)
    ref = MR.gpu_sums(f, GR.selected_tiles(f, tiles), rec)
    return film.pixels, mom, st, ref, rec, f


@pytest.mark.parametrize("which,integ,radius,crop,tiles,spp,first,count", MOMENT_CASES)
def test_moments_against_records(gpu, orc_det, which, integ, radius, crop, tiles, spp, first, count):
    px, mom, st, ref, rec, _ = _moments_case(gpu, orc_det, which, integ, radius, crop, tiles, spp, first, count)
    MR.assert_matches(px, mom, ref, "%s/%s" % (which, integ))
    assert st["camera_samples"] == ref["n"] and st["spill_samples"] == ref["n_spill"]
    assert (mom[..., 3] > 0).any() and (radius[0] == 0.5) == (ref["n_spill"] < 8)


def test_moments_chunks_at_five_samples(gpu, orc_det, monkeypatch):
    """FTN_WF_PATHS_M=1 on 813 tiles: passes of 5 samples over [3, 10) of 20 at radius 1.25, so chunk edges fall off MO_ACC_CHUNK and
    each chunk's footprints come from its own sample keys"""
    monkeypatch.setenv("FTN_WF_PATHS_M", "1")
    px, mom, st, ref, _, _ = _moments_case(gpu, orc_det, "slit", "path1", R125, FULL, None, 20, 3, 7)
    monkeypatch.delenv("FTN_WF_PATHS_M")
    MR.assert_matches(px, mom, ref, "chunked")
    assert st["camera_samples"] == ref["n"] and st["spill_samples"] == ref["n_spill"] and (mom[..., 3] > 0).any()


# ------------------------------------------------------------------ 2. the variance resolve against float64
def test_variance_against_float64(gpu, orc_det):
    """ftn_moments_resolve of the GPU's buffers against the exact variance of each pixel's mean: within resolve_bound everywhere, and
    the pixels clamped to 0 are ones whose float64 variance lies within that bound of 0 (a bright, nearly constant scene at 64 spp)"""
    N = 64
    make = lambda be: constant_sphere(be, kd=0.003, inner=True)
    smp = RandomSampler(N, 3, indexed=True)
    b, cam, res = make(gpu)
    var, film, mom, _ = M.render_moments(gpu, None, cam, res, PathIntegrator(3, 1.0), smp, scene=b.create_scene())
    rec, f, _ = MR.oracle_records(orc_det, make, PathIntegrator(3, 1.0), smp)
    ref = MR.gpu_sums(f, GR.selected_tiles(f, None), rec)
    MR.assert_matches(film.pixels, mom, ref, "near-constant")
    v64, _, absx, W = MR.variance64(f, ref, rec)
    bound = MR.resolve_bound(film.pixels, mom, absx, ref["mag_rgb"], ref["mag_sq"])
    err = np.abs(var.astype(np.float64) - v64)
    assert (err <= bound).all(), float((err / bound).max())
    clamped = var == 0
    assert clamped.any() and (~clamped & (v64 > 0)).any()
    assert (v64[clamped] <= bound[clamped]).all()


# ------------------------------------------------------------------ 3. adaptive against the simulator
ADAPTIVE_CASES = [
    # scene, integrator, N, n0, step, t, a, radius, crop, tiles, seed
    ("black", "path3", 40, 6, 0, 0.3, 0.05, R05, FULL, None, 4),
    ("black", "path3", 40, 3, 7, 0.3, 0.05, R05, FULL, None, 4),
    ("black", "path3", 40, 39, 0, 0.3, 0.05, R05, FULL, None, 4),
    ("floor_solid", "direct", 16, 2, 0, 0.3, 0.01, R05, FULL, None, 4),
    ("floor_solid", "whitted", 16, 2, 0, 0.3, 0.01, R05, FULL, None, 4),
    ("black96", "path3", 16, 4, 0, 0.3, 0.02, R125, CROP, None, 31),
    ("black96", "path3", 16, 4, 0, 0.3, 0.02, R1575, (0.0, 0.1, 0.85, 1.0), (1, 2, 0), 31),
]


def _adaptive_case(gpu, orc_det, which, integ, N, n0, step, t, a, radius, crop, tiles, seed):
    prm = AD.params(gpu, min_samples=n0, step_samples=step, threshold=t, abs_floor=a)
    b, cam, res = _camera(gpu, which)
    film, mom, cnt, info, st = AD.render_adaptive(gpu, None, cam, res, INTEGRATORS[integ](), RandomSampler(N, seed, indexed=True), prm,
                                                  scene=b.create_scene(), film=GR.film(gpu, res, crop, radius), tiles=tiles)
    rec, f, _ = MR.oracle_records(orc_det, lambda be: _camera(be, which), INTEGRATORS[integ](), RandomSampler(N, seed, indexed=True), crop, radius, tiles)
    sel = GR.selected_tiles(f, tiles)
    sim = MR.simulate(f, sel, rec, N, n0, step, t, a)
    sched = MR.schedule(n0, N, step)
    # the GPU's count of every tile: read from the counts buffer; a tile without a crop pixel converges after round 1 (the header)
    slices = MR.tile_slices(f, sel)
    gpu_n = np.array([int(cnt[ys, xs].flat[0]) if cnt[ys, xs].size else min(n0, N) for ys, xs in slices], np.int64)
    for k, (ys, xs) in enumerate(slices):
        assert (cnt[ys, xs] == gpu_n[k]).all(), k
    sure = ~sim["unsure"]
    assert np.array_equal(gpu_n[sure], sim["counts"][sure]), (gpu_n.tolist(), sim["counts"].tolist())
    for k in np.nonzero(sim["unsure"])[0]:
        assert abs(sched.index(gpu_n[k]) - sched.index(sim["counts"][k])) <= 1, k
    assert sim["unsure"].sum() <= max(2, len(sel) // 20)
    # the image: the mixed-count reference from the GPU's own counts
    kept = MR.keep_counts(rec, gpu_n)
    ref = MR.gpu_sums(f, sel, kept)
    MR.assert_matches(film.pixels, mom, ref, "%s/%s adaptive" % (which, integ))
    n_pix = np.array([cnt[ys, xs].size for ys, xs in slices], np.int64)
    assert info["rounds"] == sched.index(int(gpu_n.max())) + 1 and info["tiles"] == len(sel)
    assert info["tiles_at_max"] == int((gpu_n == N).sum()) and info["pixel_samples"] == int((gpu_n * n_pix).sum())
    assert st["camera_samples"] == len(kept) and st["spill_samples"] == ref["n_spill"]
    return gpu_n, sim, sched


@pytest.mark.parametrize("which,integ,N,n0,step,t,a,radius,crop,tiles,seed", ADAPTIVE_CASES)
def test_adaptive_against_simulator(gpu, orc_det, which, integ, N, n0, step, t, a, radius, crop, tiles, seed):
    gpu_n, sim, sched = _adaptive_case(gpu, orc_det, which, integ, N, n0, step, t, a, radius, crop, tiles, seed)
    if n0 < N:
        assert sim["rounds"] >= 2
    if radius[0] != 0.5:                                   # neighbouring tiles stop at different counts: mixed spill pixels
        assert len(set(gpu_n.tolist())) >= 2


def test_adaptive_chunks_per_round(gpu, orc_det, monkeypatch):
    """FTN_WF_PATHS_M=1 at radius 1.25 on 813 tiles: round 1 ([0, 10)) runs as two passes of 5 samples"""
    monkeypatch.setenv("FTN_WF_PATHS_M", "1")
    gpu_n, sim, _ = _adaptive_case(gpu, orc_det, "slit", "path1", 20, 10, 0, 0.1, 0.05, R125, FULL, None, 6)
    assert len(set(gpu_n.tolist())) >= 2


def test_adaptive_t0_constant_sphere(gpu, orc_det):
    _adaptive_case(gpu, orc_det, "cornell", "path", 8, 2, 3, 0.0, 0.0, R05, FULL, None, 2)
    SCENES["const"] = lambda be: constant_sphere(be, res=40)
    try:
        gpu_n, sim, _ = _adaptive_case(gpu, orc_det, "const", "path", 40, 3, 7, 0.0, 0.0, R05, FULL, None, 21)
    finally:
        del SCENES["const"]
    assert gpu_n.min() < 40
