"""The closest-hit walk over 64-byte four-box records (k_wf_trace4<.., Q64>, the default for triangle-only scenes) on the GPU (-m gpu):
films, ray counts and hit records are bit-identical with FTN_QUAD64=0 (the walk over 128-byte records) and equal to the oracle's, on the
triangle-only parity scenes, the triangle-only fuzz recipes and ray batches through ftn_intersect (tests/test_quad64_bvh.py checks the
records and the walk on the CPU)."""
import numpy as np
import pytest

from fountain_amd import PathIntegrator, RandomSampler, SceneBuilder, make_rays, scenes
from test_gpu_fuzz import build, make_recipe, render
from test_gpu_parity import SCENES, WAVE, assert_film_equal, bits, render_pair, unit_dirs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scene", ["cube_env", "cubes27"])
def test_parity_scenes_equal_with_and_without_quad64(gpu, orc_det, monkeypatch, scene):
    make, spp = SCENES[scene]
    out = {}
    for v in ("0", "1"):
        monkeypatch.setenv("FTN_QUAD64", v)
        out[v] = render_pair(gpu, orc_det, make, PathIntegrator.new(5, 1.0), RandomSampler(spp, 0, indexed=True), WAVE, "production")
    (rgb0, px0, st0), _ = out["0"]
    (rgb1, px1, st1), (rgbo, pxo, sto) = out["1"]
    assert np.array_equal(bits(px0), bits(px1)), scene
    for k in ("rays_closest", "rays_any", "camera_samples", "spill_samples"):
        assert st0[k] == st1[k] == sto[k], (k, st0[k], st1[k], sto[k])
    assert_film_equal(px1, pxo, st1["spill_samples"], scene)
    assert rgb1.mean() > 0.01


@pytest.mark.parametrize("seed", range(12))
def test_triangle_only_fuzz_equal_with_and_without_quad64(gpu, orc_det, monkeypatch, seed):
    recipe = make_recipe(seed, env_only=seed % 3 == 0, tri_only=True)
    o = build(orc_det, recipe)
    pxo, sto, erro = render(orc_det, *o, PathIntegrator.new(5, 1.0), RandomSampler(4, seed, indexed=True), WAVE)
    px = {}
    for v in ("0", "1"):
        monkeypatch.setenv("FTN_QUAD64", v)
        g = build(gpu, recipe)
        p, st, err = render(gpu, *g, PathIntegrator.new(5, 1.0), RandomSampler(4, seed, indexed=True), WAVE)
        assert err == erro
        if err is not None:
            return
        assert st["rays_closest"] == sto["rays_closest"] and st["rays_any"] == sto["rays_any"], (seed, v)
        assert_film_equal(p, pxo, st["spill_samples"], "seed %d FTN_QUAD64=%s" % (seed, v))
        px[v] = p
    assert np.array_equal(bits(px["0"]), bits(px["1"])), seed


def test_ray_batches_equal_with_and_without_quad64(gpu, orc_det, monkeypatch):
    """ftn_intersect's production walk (stats=False) over random, short and axis-parallel rays: hit distances, primitives and
    barycentrics equal bit for bit with FTN_QUAD64=0 and =1, and equal the oracle's"""
    P, N, Fc = scenes.rounded_cube_mesh()
    rng = np.random.default_rng(4)
    o = rng.uniform(-30, 30, (60000, 3)).astype(np.float32)
    d = unit_dirs(60000, 5) * rng.uniform(0.1, 40, (60000, 1)).astype(np.float32)
    d[:2000, 0] = 0.0                                                     # exceptional rays: the reference-order kernel
    d[2000:2500] *= np.float32(1e-20)                                     # |1/d| beyond the margins' range: likewise
    rays = make_rays(o, d, t_max=rng.choice([np.inf, 1.0 - 1e-4, 0.5], 60000).astype(np.float32))
    res = {}
    for v in ("0", "1"):
        monkeypatch.setenv("FTN_QUAD64", v)
        b = SceneBuilder(gpu); b.material("none"); b.shape("trianglemesh", P=P, N=N, indices=Fc)
        res[v] = b.create_scene().intersect(rays, stats=False)
    b = SceneBuilder(orc_det); b.material("none"); b.shape("trianglemesh", P=P, N=N, indices=Fc)
    to, po, bo, _ = b.create_scene().intersect(rays)
    for v in ("0", "1"):
        t, prim, bary, _ = res[v]
        assert np.array_equal(bits(t), bits(to)) and np.array_equal(prim, po), v
    assert np.array_equal(bits(res["0"][2]), bits(res["1"][2]))
    assert 0 < (po >= 0).sum() < len(po)
