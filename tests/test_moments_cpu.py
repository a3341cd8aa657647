"""The per-sample reference of the moments and of adaptive sampling (_moments_ref.py) without a GPU: the oracle's sample log, pushed
through the film rule, gives orc_render's film bit for bit; the log's order and content; its refusals; the schedule simulator's edges and
a hand-worked t = 0 case; ftn_moments_resolve (host) of the reference sums against the float64 variance of a bright, nearly constant
scene, within the first-order bound, and the pixels it clamps to 0."""
import ctypes as C

import numpy as np
import pytest

from fountain_amd import (DirectLightingIntegrator, FountainError, PathIntegrator, PerspectiveCamera, RandomSampler, SamplerIntegrator,
                          SceneBuilder, WhittedIntegrator, scenes, _abi as A)
from fountain_amd import moments as M

import _gbuffer_ref as GR
import _moments_ref as MR

F32 = np.float32
bits = MR.bits
INTEGRATORS = {"path": lambda: PathIntegrator(5, 1.0), "direct": lambda: DirectLightingIntegrator(4), "whitted": lambda: WhittedIntegrator(4)}


def constant_sphere(be, res=24, L=(0.7, 1.3, 2.1), kd=0.0, inner=False):
    """test_moments.constant_sphere (the camera inside a black-matte emitting sphere: every camera sample returns L); with kd > 0 the
    emitter reflects a little of its own light, and `inner` adds a grey sphere in view: bright and nearly constant"""
    b = SceneBuilder(be)
    b.attribute_begin()
    b.material("matte", Kd=(kd, kd, kd))
    b.area_light_source("diffuse", L=L)
    b.reverse_orientation()
    b.shape("sphere", radius=50.0)
    b.attribute_end()
    if inner:
        b.attribute_begin(); b.material("matte", Kd=(0.5, 0.5, 0.5)); b.shape("sphere", radius=0.3); b.attribute_end()
    cam = PerspectiveCamera.look_at(be, (0, -2, 0), (0, 0, 0), (0, 0, 1), (res, res), fov=60.0)
    return b, cam, (res, res)


# ------------------------------------------------------------------ 1. the sample log reproduces orc_render
FILMS = [((0.5, 0.5), (0.0, 0.0, 1.0, 1.0), None),
         ((1.25, 1.25), (0.1, 0.05, 0.9, 0.95), None),
         ((1.5, 0.75), (0.0, 0.1, 0.85, 1.0), (1, 2, 0)),
         ((1.25, 1.25), (0.0, 0.0, 1.0, 1.0), (2, 3, 5))]
RANGES = [(4, 0, 0), (20, 3, 13)]


@pytest.mark.parametrize("integ", sorted(INTEGRATORS))
@pytest.mark.parametrize("radius,crop,tiles", FILMS)
@pytest.mark.parametrize("spp,first,count", RANGES)
def test_sample_log_reproduces_orc_render(orc_det, integ, radius, crop, tiles, spp, first, count):
    """the records through oracle_film equal orc_render's film on every pixel, bit for bit (the oracle sums serially: no spill
    tolerance), and the statistics' sample counts follow from the records' footprints"""
    b, cam, res = scenes.cornell(orc_det, res=40)
    sc = b.create_scene()
    smp = RandomSampler(spp, 7, indexed=True, first_sample=first, sample_count=count)
    f = GR.film(orc_det, res, crop, radius)
    rec, st = MR.sample_log(orc_det, sc, cam, f, INTEGRATORS[integ](), smp, tiles)
    want = GR.film(orc_det, res, crop, radius)
    st_want = SamplerIntegrator(cam, INTEGRATORS[integ]()).render_parallel(sc, want, smp, tiles=tiles, n_threads=16)
    sel = GR.selected_tiles(f, tiles)
    got = MR.oracle_film(f, sel, rec)
    assert np.array_equal(bits(got), bits(want.pixels)), int((bits(got) != bits(want.pixels)).any(-1).sum())
    ref = MR.gpu_sums(f, sel, rec)
    assert len(rec) == st["camera_samples"] == st_want["camera_samples"] == ref["n"]
    assert st["spill_samples"] == st_want["spill_samples"] == ref["n_spill"]
    assert (radius[0] == 0.5) == (ref["n_spill"] < 8)
    assert np.array_equal(bits(ref["beauty"][..., 3]), bits(want.pixels[..., 3]))        # integer weights: any order


def test_sample_log_order_and_content(orc_det):
    """selected-tile order, row-major pixels within a tile, increasing sample index; p_film is the pixel plus the first two draws of
    the sample's indexed stream; ray_weight 1 (perspective camera); the record count query; refusals"""
    spp, first, count, seed, tiles = 20, 3, 13, 9, (1, 3, 0)
    b, cam, res = scenes.cornell(orc_det, res=40)
    sc = b.create_scene()
    f = GR.film(orc_det, res, (0.05, 0.0, 1.0, 0.9), (1.25, 1.25))
    integ = PathIntegrator(2, 1.0)
    rec, _ = MR.sample_log(orc_det, sc, cam, f, integ, RandomSampler(spp, seed, indexed=True, first_sample=first, sample_count=count), tiles)
    sel = GR.selected_tiles(f, tiles)
    want = [(k, x, y, s) for k, (x0, y0, x1, y1) in enumerate(sel) for y in range(y0, y1) for x in range(x0, x1) for s in range(first, first + count)]
    assert len(rec) == len(want)
    assert np.array_equal(np.stack([rec["tile"], rec["px"], rec["py"], rec["sample"]], -1), np.array(want))
    u5 = (C.c_float * 5)()
    for r in rec[:: max(1, len(rec) // 97)]:
        orc_det.lib.orc_kat_indexed_f32(C.c_uint64(seed), C.c_int32(int(r["px"])), C.c_int32(int(r["py"])), C.c_uint32(int(r["sample"])), u5, C.c_size_t(5))
        assert bits(r["p_film"]).tolist() == bits([F32(r["px"]) + F32(u5[0]), F32(r["py"]) + F32(u5[1])]).tolist()
    assert (rec["ray_weight"] == 1).all() and np.isfinite(rec["L"]).all() and (rec["L"] > 0).any()
    fn = orc_det.lib.orc_render_sample_log
    tr = A.ftn_tile_range()
    n = C.c_size_t()
    args = [sc.handle, C.byref(cam.desc), C.byref(f.desc), None, C.byref(integ.desc), C.byref(tr), 1]
    args[3] = C.byref(RandomSampler(4, 0).desc)                                              # FTN_SAMPLER_TILE_SERIAL
    assert fn(*args, None, 0, C.byref(n), None, None) == A.FTN_ERR_UNSUPPORTED
    args[3] = C.byref(RandomSampler(4, 0, indexed=True).desc)
    assert fn(*args, None, 0, C.byref(n), None, None) == 0 and n.value == 4 * sum(
        (t[2] - t[0]) * (t[3] - t[1]) for t in GR.selected_tiles(f, None))
    small = np.zeros(n.value - 1, MR.RECORD)
    assert fn(*args, small.ctypes.data_as(C.c_void_p), C.c_size_t(len(small)), C.byref(n), None, None) == A.FTN_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------ 2. the schedule simulator
def test_simulator_edges(orc_det):
    from test_adaptive import sphere_on_black
    assert MR.schedule(3, 40, 7) == [3, 10, 17, 24, 31, 38, 40]
    assert MR.schedule(6, 40, 0) == [6, 12, 24, 40] and MR.schedule(39, 40, 0) == [39, 40] and MR.schedule(40, 40, 0) == [40]
    N = 40
    rec, f, _ = MR.oracle_records(orc_det, lambda be: sphere_on_black(be, 64), PathIntegrator(3, 1.0), RandomSampler(N, 4, indexed=True))
    sel = GR.selected_tiles(f, None)
    one = MR.simulate(f, sel, rec, N, N, 0, 0.05, 0.01)                   # n0 = N: one round, every tile at N
    assert one["rounds"] == 1 and (one["counts"] == N).all() and not one["unsure"].any()
    huge = MR.simulate(f, sel, rec, N, 3, 0, 1e15, 1.0)                    # every tile passes after round 1
    assert huge["rounds"] == 1 and (huge["counts"] == 3).all()
    zero = MR.simulate(f, sel, rec, N, 3, 7, 1e-9, 0.0)                    # the lit tiles never pass: the clipped schedule to N
    assert zero["rounds"] == 7 and set(zero["counts"].tolist()) == {3, N}
    mid = MR.simulate(f, sel, rec, N, 6, 0, 0.3, 0.05)
    assert set(mid["counts"].tolist()) == {6, 12, 24, 40} and mid["rounds"] == 4
    # a tile's count is the first schedule entry at which all of its pixels pass, on the sums of the records kept so far
    for n in (6, 12, 24):
        counts = np.where(mid["counts"] >= n, n, mid["counts"])
        ref = MR.gpu_sums(f, sel, MR.keep_counts(rec, counts))
        ok = MR.criterion_ref(ref["beauty"], ref["moments"], 0.3, 0.05)
        for k, (ys, xs) in enumerate(MR.tile_slices(f, sel)):
            if mid["counts"][k] >= n and not mid["unsure"][k]:
                assert bool(ok[ys, xs].all()) == (mid["counts"][k] == n), (k, n)


def test_simulator_t0_constant_sphere(orc_det):
    """every sample returns c: by hand, a pixel with n samples holds S = n-fold float32 sums of c pushed through rgb_to_xyz and
    sq_y = the n-fold sum of fl(Y * Y); at t = 0 it passes iff the resolved v is exactly 0.  A plain per-tile loop over the schedule
    gives the counts the simulator must give."""
    N, n0, step = 40, 3, 7
    L = (0.7, 1.3, 2.1)
    rec, f, _ = MR.oracle_records(orc_det, lambda be: constant_sphere(be, res=40, L=L), PathIntegrator(5, 1.0), RandomSampler(N, 21, indexed=True))
    c = np.array(L, F32)
    assert np.array_equal(bits(rec["L"]), bits(np.broadcast_to(c, rec["L"].shape)))
    sel = GR.selected_tiles(f, None)
    Y = MR.rgb_to_xyz(c)[1]

    def passes(n):
        R, sq = np.zeros(3, F32), F32(0)
        for _ in range(n):
            R, sq = (R + c).astype(F32), F32(sq + F32(Y * Y))
        pix = np.concatenate([F32(0) + MR.rgb_to_xyz(R), [F32(n)]]).astype(F32)
        return bool(MR.criterion_ref(pix, np.array([0, 0, 0, sq], F32), 0.0, 0.0))
    want = np.zeros(len(sel), np.int64)
    active = np.ones(len(sel), bool)
    for n in MR.schedule(n0, N, step):
        want[active] = n
        for k in np.nonzero(active)[0]:                    # every crop pixel of the tile holds n own samples (radius 0.5)
            if n < N and passes(n):
                active[k] = False
        if not active.any():
            break
    sim = MR.simulate(f, sel, rec, N, n0, step, 0.0, 0.0)
    assert np.array_equal(sim["counts"], want) and not sim["unsure"].any()
    assert min(want) < N                                   # some count reaches v == 0 before N


# ------------------------------------------------------------------ 3. the resolve against float64
def test_resolve_against_float64(orc_det, ftn):
    """ftn_moments_resolve (host; the device shares its code) of the reference sums against the exact variance of each pixel's mean:
    within resolve_bound everywhere; every pixel it clamps to 0 has a float64 variance within that bound of 0; a bright, nearly
    constant scene at 64 spp has such pixels beside pixels it does not clamp"""
    N = 64
    rec, f, _ = MR.oracle_records(orc_det, lambda be: constant_sphere(be, kd=0.003, inner=True), PathIntegrator(3, 1.0),
                                  RandomSampler(N, 3, indexed=True))
    sel = GR.selected_tiles(f, None)
    ref = MR.gpu_sums(f, sel, rec)
    var = M.resolve(ftn, ref["beauty"], ref["moments"])
    v64, mean, absx, W = MR.variance64(f, ref, rec)
    bound = MR.resolve_bound(ref["beauty"], ref["moments"], absx, ref["mag_rgb"], ref["mag_sq"])
    assert (W == N).all()
    err = np.abs(var.astype(np.float64) - v64)
    assert (err <= bound).all(), float((err / bound).max())
    clamped = var == 0
    assert clamped.any() and (~clamped & (v64 > 0)).any()
    assert (v64[clamped] <= bound[clamped]).all()


def test_resolve_precision_limit(ftn):
    """the header's precision limit on synthetic 64-sample pixels (radius 0.5 sums: own samples from +0 in sample order): a Y variance of
    2^-21 mean^2 already comes out as 0 in some pixels, and r, g, b, which the resolve recovers through the beauty's xyz, clamp at
    variances far above that; every result lies within resolve_bound of the float64 variance"""
    rng = np.random.default_rng(0)
    W, n = 64, 2000
    for lg, what in ((-21, 3), (-18, 0)):
        base = rng.uniform(0.2, 3.0, (n, 3)).astype(F32)
        L = (base[:, None, :] * (1 + 2.0 ** (lg / 2) * rng.standard_normal((n, W, 3)))).astype(F32)
        s, q = np.zeros((n, 3), F32), np.zeros((n, 4), F32)
        for i in range(W):
            y = MR.rgb_to_xyz(L[:, i])[:, 1]
            s = (s + L[:, i]).astype(F32)
            q = (q + np.concatenate([L[:, i] * L[:, i], (y * y)[:, None]], -1).astype(F32)).astype(F32)
        px = np.concatenate([F32(0) + MR.rgb_to_xyz(s), np.full((n, 1), W, F32)], -1).astype(F32)
        var = M.resolve(ftn, px, q)
        x = np.concatenate([L.astype(np.float64), MR.rgb_to_xyz(L)[..., 1:2].astype(np.float64)], -1)
        v64 = x.var(1, ddof=1) / W
        bound = MR.resolve_bound(px, q, np.abs(x).sum(1), np.abs(x[..., :3]).sum(1), (x * x).sum(1))
        assert (np.abs(var - v64) <= bound).all()
        clamped = var[:, what] == 0
        assert clamped.any() and (v64[clamped, what] * W >= 2.0 ** (lg - 1) * (x[clamped, :, what].mean(1) ** 2)).any(), lg
