"""The path, direct-lighting and Whitted integrators of both oracle builds (oracle/orc_render.hpp; libm and deterministic math) against the binary64
restatement of the reference's Rust (tests/_integrator_ref.py), sample by sample, and against properties no reading of the reference enters (DESIGN.md
3.5).  The device runs the same comparisons in tests/test_integrator.py."""
import numpy as np
import pytest

import _gbuffer_ref as GR
import _integrator_common as K
import _integrator_ref as IG
import _moments_ref as MR


@pytest.fixture(params=["orc", "orc_det"])
def oracle(request):
    return request.getfixturevalue(request.param)


def oracle_pixels(oracle):
    return lambda make, integ, spp, seed: K.oracle_pixels(oracle, make, integ, spp, seed)


# ------------------------------------------------------------------ layer 1
def test_sampler_in_integers():
    """the vectorised generator against Python integers: key, SplitMix64 seeding, Xoshiro256+, the upper 24 bits; large coordinates and seeds"""
    px, py, s = np.array([0, 3, 1023, 65535, 7]), np.array([0, 5, 4095, 1, 1048575]), np.array([0, 2, 255, 65535, 9])
    for seed in (0, 7, 2 ** 63 + 12345, 2 ** 64 - 1):
        rng = IG.Rng(seed, px, py, s)
        got = np.stack([rng.f(np.arange(5)) for _ in range(12)], axis=1)
        want = np.array([IG.scalar_floats(seed, int(x), int(y), int(k), 12) for x, y, k in zip(px, py, s)])
        assert np.array_equal(got, want)
        assert (got >= 0).all() and (got < 1).all() and np.array_equal(got, got.astype(np.float32))


@pytest.mark.parametrize("name", sorted(K.CONFIGS))
def test_oracle_against_restatement(oracle, name):
    cfg, ref = K.CONFIGS[name], K.restated(name)
    share = float(ref["fragile"].mean())
    assert share <= K.MAX_FRAGILE_SHARE, (name, share)
    assert ref["error"] == cfg.error
    if cfg.error:                                     # a hit without a material under direct lighting and Whitted: unimplemented!()
        assert K.error_code(lambda: K.logged(oracle, cfg)) == cfg.error
        return
    rec, st = K.logged(oracle, cfg)
    assert st["spill_samples"] == 0 and st["camera_samples"] == len(rec) == len(ref["L"])
    p999, worst, share = K.compare(cfg, ref, rec)
    print("%s: 99.9th percentile %.3e, maximum %.3e, left out %.2f %%" % (name, p999, worst, 100.0 * share))
    K.ray_counts_agree(cfg, ref, st)
    bound = K.TOLERANCE[name]
    assert p999 <= bound[0] and worst <= bound[1], (name, p999, worst, bound)


def test_measured_table_is_the_libm_oracles(orc):
    """MEASURED holds what the libm oracle gives on this restatement (to the digits written), for every configuration"""
    assert sorted(K.MEASURED) == sorted(k for k, c in K.CONFIGS.items() if not c.error)
    for name, (p, m, share) in K.MEASURED.items():
        got = K.compare(K.CONFIGS[name], K.restated(name), K.logged(orc, K.CONFIGS[name])[0])
        assert np.allclose(got, (p, m, share), rtol=5.0e-3, atol=1.0e-12), (name, got, (p, m, share))


def test_configurations_reach_their_edges():
    r = K.restated
    assert r("dim_box_d12")["roulette_cut"].sum() > 100 and not r("box_d5_rr0")["roulette_cut"].any() and not r("box_d2")["roulette_cut"].any()
    # without lights uniform_sample_one_light returns before it draws: 5 draws for the camera, 2 per bounce
    assert (r("dark_path")["draws"] % 2 == 1).all() and r("dark_path")["draws"].max() == 5 + 2 * 3 and not r("dark_path")["L"].any()
    # the sheet does not count as a bounce: more closest-hit rays than max_depth + 1 + one per light sample
    assert r("sheet_path")["rays_closest"].max() > r("box_d2")["rays_closest"].max() + 1
    # emission seen only through specular bounces; the direct-lighting chain runs to its limit
    assert r("corridor_path")["L"].max() >= 9.0 * 0.8 ** 5 and r("corridor_direct")["rays_closest"].max() == 5
    assert r("box_d0")["rays_any"].sum() == 0 and r("box_d0")["L"].max() == 12.0
    for name in K.CONFIGS:
        if not K.CONFIGS[name].error and not name.startswith("dark"):
            assert r(name)["L"].mean() > 1.0e-3, name


def test_no_material_mixes_specular_with_other_lobes():
    """why estimate_direct's scattering pdf may be asked with either flag set (the mutation table): every material's lobes are all
    specular or none is, so BxDFType::all() and all() & !SPECULAR match the same lobes wherever f is not black.  A material that mixes them would
    need a test of its own."""
    import _bsdf_common as BK
    import _bsdf_ref as B
    for kind, params in [(c[1], c[2]) for c in BK.BY_NAME.values()]:
        for multiple in (False, True):
            lobes = B.material_lobes(kind, multiple, **params)
            if lobes:
                assert len({bool(l.type & B.SPECULAR) for l in lobes}) == 1, (kind, params)


@pytest.mark.parametrize("name", ["cornell_path", "gallery_direct", "corridor_whitted", "image_path"])
def test_one_sample_films_hold_the_log(orc_det, name):
    """the observation the device tests rely on: a one-sample range on a box film of radius 0.5 leaves rgb_to_xyz(0 + L) in every pixel"""
    cfg = K.CONFIGS[name]
    xyz, tot = K.one_sample_films(orc_det, cfg)
    rec, st = K.logged(orc_det, cfg)
    assert np.array_equal(GR.bits(xyz), GR.bits(MR.rgb_to_xyz(rec["L"])))
    assert all(tot[k] == st[k] for k in tot)


# ------------------------------------------------------------------ layer 2
@pytest.mark.parametrize("name", K.SCALING)
def test_exact_scaling(oracle, name):
    cfg = K.CONFIGS[name]

    def render(make):
        b, cam, res = make(oracle)
        rec, st = MR.sample_log(oracle, b.create_scene(), cam, GR.film(oracle, res), cfg.integrator(), cfg.sampler())
        return rec["L"].copy(), st
    K.check_exact_scaling(cfg, render)


@pytest.mark.parametrize("light,integ", K.MEAN_PARAMS)
def test_means_against_quadrature(oracle, light, integ):
    share = K.check_mean_case(oracle_pixels(oracle), light, integ)
    print("%s/%s: 5 sigma of the image mean is %.3f %% of it at %d samples per pixel" % (light, integ, 100.0 * share, K.MEAN_CASES[light]))


@pytest.mark.parametrize("receiver,R,integ", K.MIS_PARAMS)
def test_mis_does_not_move_the_mean(oracle, receiver, R, integ):
    share = K.check_mis_case(oracle_pixels(oracle), receiver, R, integ)
    print("%s/%s/%s: 5 sigma of the image mean is %.3f %% of it at %d samples per pixel" % (receiver, R, integ, 100.0 * share, K.MIS_CASES[(receiver, R)]))


def test_estimators_agree(oracle):
    K.check_estimators_agree(oracle_pixels(oracle))


def test_roulette_is_unbiased(oracle):
    K.check_roulette_unbiased(oracle_pixels(oracle))
