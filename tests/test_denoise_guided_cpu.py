"""The host twin of the variance-guided a-trous denoiser (ftn_denoise_guided_cpu, include/fountain_hip_denoise_guided.h) against an
independent float64 numpy restatement of the header's text (tests/_denoise_guided_ref.py), and the properties the definition implies:
an exact copy at 0 levels, constant colour as a fixed point, scale equivariance bit for bit, noise-free pass-through, geometry alone
under unknown variance, non-finite and negative inputs, zero-weight taps next to infinite variance, no dependence on the host thread
count, and a filter strength that follows the noise level.  CPU only."""
import os

import numpy as np
import pytest

from fountain_amd import denoise as D

import _denoise_guided_ref as GR
import _denoise_ref as DR

SIZES = [(1, 1), (3, 5), (9, 17), (48, 64), (120, 200)]          # (h, w)
LEVELS = [(1, 1), (2, 0), (3, 1), (5, 0), (5, 1), (10, 0), (10, 1)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_close(got, want, rtol=1e-5):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    err = np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-30)
    assert err.size == 0 or err.max() <= rtol, "max relative error %.3g" % err.max()


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("levels,flags", LEVELS)
def test_twin_equals_the_restatement(ftn, h, w, levels, flags):
    rgb, gb, var4, _ = GR.synthetic(h, w, seed=1000 * h + w + levels)
    p = dict(levels=levels, flags=flags)
    assert_close(D.denoise_guided_cpu(ftn, rgb, gb, var4, p), GR.reference(rgb, gb, var4, **p))


def test_twin_equals_the_restatement_other_parameters(ftn):
    rgb, gb, var4, _ = GR.synthetic(48, 64, seed=4)
    for p in (dict(levels=4, sigma_variance=1.5, sigma_normal=0.9, sigma_plane=0.03, albedo_eps=0.25, rel_eps=0.0),
              dict(levels=3, sigma_variance=0.5, rel_eps=0.05), dict(levels=6, sigma_variance=8.0, sigma_plane=0.1, flags=0)):
        assert_close(D.denoise_guided_cpu(ftn, rgb, gb, var4, p), GR.reference(rgb, gb, var4, **p))


@pytest.mark.parametrize("h,w", SIZES)
def test_zero_levels_is_an_exact_copy(ftn, h, w):
    rgb, gb, var4, _ = GR.synthetic(h, w, seed=7)
    rgb.reshape(-1)[::7] = np.nan
    rgb.reshape(-1)[3::11] = -np.inf
    var4.reshape(-1)[::5] = np.nan
    for flags in (0, 1):
        assert np.array_equal(bits(D.denoise_guided_cpu(ftn, rgb, gb, var4, dict(levels=0, flags=flags))), bits(rgb))


@pytest.mark.parametrize("kind", ["flat", "normal", "coverage", "planes"])
def test_constant_colour_is_a_fixed_point(ftn, kind):
    gb = DR.gbuffer(64, 48, None, kind)
    gb[..., 0:3] = 0.5
    gb[gb[..., 10] == 0, 0:3] = 0.0
    rgb = np.full((64, 48, 3), 0.3, np.float32)
    var4 = np.random.default_rng(1).uniform(0.0, 0.1, (64, 48, 4)).astype(np.float32)
    for flags in (0, 1):
        for levels in (5, 10):
            out = D.denoise_guided_cpu(ftn, rgb, gb, var4, dict(levels=levels, flags=flags))
            assert np.abs(out / rgb - 1).max() <= 1e-6, (flags, levels)


@pytest.mark.parametrize("k", [-3, -1, 1, 2, 5])
@pytest.mark.parametrize("flags", [0, 1])
def test_scale_equivariance(ftn, k, flags):
    """out(2^k rgb, gb, 4^k var4) == 2^k out(rgb, gb, var4), bit for bit: every term of the colour distance is homogeneous"""
    rgb, gb, var4, _ = GR.synthetic(48, 64, seed=12)
    var4[5:9, 5:9] = np.inf
    for p in (dict(flags=flags), dict(flags=flags, rel_eps=0.01, levels=7)):
        base = D.denoise_guided_cpu(ftn, rgb, gb, var4, p)
        s = np.float32(2.0 ** k)
        scaled = D.denoise_guided_cpu(ftn, rgb * s, gb, var4 * np.float32(4.0 ** k), p)
        assert np.array_equal(bits(scaled), bits(base * s))
        assert not np.array_equal(bits(base), bits(rgb))


def test_noise_free_pass_through(ftn):
    """var4 = 0 and rel_eps = 0: no two different colours mix, so an image whose neighbours all differ comes back within a few ulps;
    ftn_denoise at its defaults blurs the same image"""
    gb = DR.gbuffer(40, 64, None, "flat")
    rgb = np.random.default_rng(5).uniform(0.2, 0.8, (40, 64, 3)).astype(np.float32)
    var4 = np.zeros((40, 64, 4), np.float32)
    for flags in (0, 1):
        out = D.denoise_guided_cpu(ftn, rgb, gb, var4, dict(flags=flags, rel_eps=0.0, levels=10))
        assert np.abs(out / rgb - 1).max() <= 4 * 2.0 ** -24, np.abs(out / rgb - 1).max()
    assert np.abs(D.denoise_cpu(ftn, rgb, gb) / rgb - 1).max() > 0.05
    assert np.abs(D.denoise_guided_cpu(ftn, rgb, gb, var4) / rgb - 1).max() > 1e-6          # (the default rel_eps lets close colours mix)


def test_unknown_variance_is_geometry_alone(ftn):
    """var4 = +inf everywhere (fewer than 2 samples): every colour term is 0 and geometry alone decides"""
    rgb, gb, _, _ = GR.synthetic(48, 64, seed=31)
    inf = np.full((48, 64, 4), np.inf, np.float32)
    for flags in (0, 1):
        got = D.denoise_guided_cpu(ftn, rgb, gb, inf, dict(flags=flags))
        assert_close(got, GR.reference(rgb, gb, inf, geometry_only=True, flags=flags))
        assert np.isfinite(got).all()
    one = GR.synthetic(48, 64, seed=31, samples=1)
    assert np.isinf(one[2]).all()
    assert np.array_equal(bits(D.denoise_guided_cpu(ftn, one[0], one[1], one[2])), bits(D.denoise_guided_cpu(ftn, one[0], one[1], inf)))


def test_non_finite_and_negative_inputs(ftn):
    """a non-finite colour, or a NaN or negative variance, is copied through (remodulated) and ignored by its neighbours; an infinite
    variance is usable and carries through; non-finite features weigh 0"""
    rgb, gb, var4, _ = GR.synthetic(48, 64, seed=21)
    rgb[10, 10] = (np.nan, 0.2, 0.3)
    rgb[20, 30] = (np.inf, 1.0, 1.0)
    rgb[40, 60] = np.nan
    var4[12, 12, 0] = np.nan
    var4[14, 40, 1] = -1e-3
    var4[30, 20, 2] = np.inf
    var4[36:40, 4:8] = np.inf
    gb[5, 40, 3] = np.nan
    gb[25, 20, 6] = np.inf
    for flags in (0, 1):
        out = D.denoise_guided_cpu(ftn, rgb, gb, var4, dict(flags=flags))
        assert_close(out, GR.reference(rgb, gb, var4, flags=flags))
        assert np.isnan(out[10, 10, 0]) and np.isnan(out[40, 60]).all() and out[20, 30, 0] == np.inf
        bad = ~np.isfinite(rgb).all(-1)
        assert np.isfinite(out[~bad]).all()
        one = D.denoise_guided_cpu(ftn, rgb, gb, var4, dict(flags=flags, levels=1))
        for y, x in ((12, 12), (14, 40)):                                # not changed: every level keeps u (remodulated alike)
            assert np.array_equal(bits(out[y, x]), bits(one[y, x]))
            assert np.abs(out[y, x] / rgb[y, x] - 1).max() <= 2 * 2.0 ** -24


@pytest.mark.parametrize("t_target,above", [(95.0, False), (104.0, False), (104.0, True)])
def test_zero_and_subnormal_weights_next_to_infinite_variance(ftn, t_target, above):
    """the one-tap image of _denoise_ref.one_tap, with the bright neighbour's variance +inf: its weight is a binary32 subnormal (t about
    95) whose square is 0, or it is 0 (t beyond 104).  Neither may turn the centre's propagated variance into NaN, which would keep the
    centre out of the next level; pixel 0, covered here, takes the centre at level 1."""
    rgb, gb, p, t, _ = DR.one_tap(t_target, above)
    gb[0, 0, 10] = 1.0                                                   # pixel 0 joins the plane: it sees the centre at step 2
    gb[0, 0, 3:6] = (0.0, 0.0, 1.0)
    var4 = np.full((1, 5, 4), 0.01, np.float32)
    var4[0, 3] = np.inf
    params = dict(levels=2, flags=0, sigma_normal=1.0, sigma_variance=1e3)
    got = D.denoise_guided_cpu(ftn, rgb, gb, var4, params)
    want = GR.reference(rgb, gb, var4, **params)
    assert_close(got, want)
    assert np.isfinite(got).all()
    assert got[0, 0, 0] < 0.5                                            # pixel 0 mixed with the black centre


def test_result_does_not_depend_on_the_thread_count(ftn):
    rgb, gb, var4, _ = GR.synthetic(640, 640, seed=3)                    # 409,600 pixels: parallel_for uses up to 7 threads
    old = os.environ.get("FTN_BVH_THREADS")
    got = {}
    try:
        for nt in (1, 7):
            os.environ["FTN_BVH_THREADS"] = str(nt)
            got[nt] = D.denoise_guided_cpu(ftn, rgb, gb, var4, dict(levels=3))
    finally:
        if old is None: os.environ.pop("FTN_BVH_THREADS", None)
        else: os.environ["FTN_BVH_THREADS"] = old
    assert np.array_equal(bits(got[1]), bits(got[7]))


def test_filter_strength_follows_the_noise_level(ftn):
    """one plane, one clean colour, noise amplitude 8x in the left half and 1x in the right (var4 to match): the guided filter removes
    about the same share of the noise in both halves; ftn_denoise, which guesses the noise from brightness, is far from that"""
    h, w = 96, 128
    amp = np.where(np.arange(w)[None, :] < w // 2, 8.0, 1.0) * np.ones((h, 1))
    rgb, gb, var4, clean = GR.synthetic(h, w, seed=8, kind="flat", amplitude=amp)
    left, right = np.s_[:, 4:w // 2 - 4], np.s_[:, w // 2 + 4:w - 4]
    mse = lambda img, s: float(((img[s].astype(np.float64) - clean[s]) ** 2).mean())
    ratios = {}
    for name, out in (("guided", D.denoise_guided_cpu(ftn, rgb, gb, var4)), ("unguided", D.denoise_cpu(ftn, rgb, gb))):
        ratios[name] = (mse(out, left) / mse(rgb, left), mse(out, right) / mse(rgb, right))
    print("residual / input MSE, 8x half and 1x half: guided %.4g, %.4g; unguided %.4g, %.4g" % (ratios["guided"] + ratios["unguided"]))
    g = ratios["guided"]
    assert max(g) <= 0.02
    assert max(g) / min(g) <= 4.0
    assert ratios["unguided"][0] > 10 * g[0]
