"""The device's path, direct-lighting and Whitted integrators (the megakernel's path_li / direct_li / estimate_direct, the wavefront pipeline's k_wf_shade,
k_wf_shade_dl, pending MIS terms and k_wf_accumulate) through all three kernel settings: sample by sample and bit for bit against the deterministic
oracle's sample log on every configuration of tests/_integrator_common.py, whose log test_integrator_cpu.py holds against the binary64 restatement (the
bounds are checked here again on the log the device equals), and against the properties of layer 2 with the seeds and bounds of the CPU tests
(DESIGN.md 3.5).  One sample is observed through a one-sample range of the indexed sampler on a box film of radius 0.5."""
import numpy as np
import pytest

from fountain_amd import SamplerIntegrator

import _gbuffer_ref as GR
import _integrator_common as K
import _moments_ref as MR

pytestmark = pytest.mark.gpu
SETTINGS = sorted(K.SETTINGS)


def device_pixels(gpu, setting):
    return lambda make, integ, spp, seed: K.device_pixels(gpu, make, integ, spp, seed, setting)


# ------------------------------------------------------------------ layer 3 (and the bounds of layer 1 on the log the device equals)
@pytest.fixture(scope="module")
def logs(orc_det):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = K.logged(orc_det, K.CONFIGS[name])
        return cache[name]
    return get


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("name", sorted(K.CONFIGS))
def test_device_equals_the_oracle_per_sample(gpu, orc_det, logs, name, setting):
    cfg = K.CONFIGS[name]
    if cfg.error:
        assert K.error_code(lambda: K.one_sample_films(gpu, cfg, setting)) == cfg.error == K.error_code(lambda: K.logged(orc_det, cfg))
        return
    rec, st = logs(name)
    xyz, tot = K.one_sample_films(gpu, cfg, setting)
    want = MR.rgb_to_xyz(rec["L"])
    differs = (GR.bits(xyz) != GR.bits(want)).any(axis=1)
    assert not differs.any(), (name, setting, int(differs.sum()), np.flatnonzero(differs)[:8])
    for k in ("rays_closest", "rays_any", "camera_samples"):
        assert tot[k] == st[k], (name, setting, k, tot[k], st[k])
    ref = K.restated(name)
    assert float(ref["fragile"].mean()) <= K.MAX_FRAGILE_SHARE
    p999, worst, _ = K.compare(cfg, ref, rec)
    assert p999 <= K.TOLERANCE[name][0] and worst <= K.TOLERANCE[name][1], (name, p999, worst)


# ------------------------------------------------------------------ layer 2
@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("name", K.SCALING)
def test_exact_scaling(gpu, name, setting):
    """the whole film (its sums of scaled samples scale exactly too) and the ray counts"""
    cfg = K.CONFIGS[name]

    def render(make):
        b, cam, res = make(gpu)
        film = GR.film(gpu, res)
        st = SamplerIntegrator(cam, cfg.integrator()).render_parallel(b.create_scene(), film, cfg.sampler(), **K.SETTINGS[setting])
        assert st["spill_samples"] == 0 and np.all(film.pixels[..., 3] == cfg.spp)
        return film.pixels[..., :3].copy(), st
    K.check_exact_scaling(cfg, render)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("light,integ", K.MEAN_PARAMS)
def test_means_against_quadrature(gpu, light, integ, setting):
    K.check_mean_case(device_pixels(gpu, setting), light, integ)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("receiver,R,integ", K.MIS_PARAMS)
def test_mis_does_not_move_the_mean(gpu, receiver, R, integ, setting):
    K.check_mis_case(device_pixels(gpu, setting), receiver, R, integ)


@pytest.mark.parametrize("setting", SETTINGS)
def test_estimators_agree(gpu, setting):
    K.check_estimators_agree(device_pixels(gpu, setting))


@pytest.mark.parametrize("setting", SETTINGS)
def test_roulette_is_unbiased(gpu, setting):
    K.check_roulette_unbiased(device_pixels(gpu, setting))


@pytest.mark.parametrize("setting", SETTINGS)
def test_a_scene_without_lights_is_exactly_zero(gpu, setting):
    for name in ("dark_path", "dark_direct"):
        xyz, _ = K.one_sample_films(gpu, K.CONFIGS[name], setting)
        assert not xyz.any()
