"""The host twin of the a-trous denoiser (ftn_denoise_cpu, include/fountain_hip_denoise.h) against an independent float64 numpy
restatement of the filter's text (tests/_denoise_ref.py), and its properties at default parameters: an exact copy at 0 levels, fixed
points, edges kept, albedo edges carried through demodulation, noise reduced, no dependence on the host thread count, non-finite
inputs, subnormal weights.  CPU only."""
import os

import numpy as np
import pytest

from fountain_amd import denoise as D

import _denoise_ref as R

SIZES = [(1, 1), (3, 5), (9, 17), (48, 64), (120, 200)]          # (h, w)


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
@pytest.mark.parametrize("levels,flags", [(1, 1), (3, 0), (5, 1), (5, 0), (10, 1)])
def test_twin_equals_the_restatement(ftn, h, w, levels, flags):
    rgb, gb, _ = R.synthetic(h, w, seed=1000 * h + w + levels)
    got = D.denoise_cpu(ftn, rgb, gb, dict(levels=levels, flags=flags))
    assert_close(got, R.reference(rgb, gb, levels=levels, flags=flags))


def test_twin_equals_the_restatement_other_parameters(ftn):
    rgb, gb, _ = R.synthetic(48, 64, seed=4)
    p = dict(levels=4, sigma_color=0.7, sigma_normal=0.9, sigma_plane=0.03, albedo_eps=0.25, color_eps=0.0)
    assert_close(D.denoise_cpu(ftn, rgb, gb, p), R.reference(rgb, gb, **p))


@pytest.mark.parametrize("h,w", SIZES)
def test_zero_levels_is_an_exact_copy(ftn, h, w):
    rgb, gb, _ = R.synthetic(h, w, seed=7)
    rgb.reshape(-1)[:: 7] = np.nan
    rgb.reshape(-1)[3:: 11] = -np.inf
    for flags in (0, 1):
        assert np.array_equal(bits(D.denoise_cpu(ftn, rgb, gb, dict(levels=0, flags=flags))), bits(rgb))


@pytest.mark.parametrize("kind", ["flat", "normal", "coverage", "planes"])
def test_constant_colour_is_a_fixed_point(ftn, kind):
    gb = R.gbuffer(64, 48, None, kind)
    gb[..., 0:3] = 0.5
    gb[gb[..., 10] == 0, 0:3] = 0.0
    rgb = np.full((64, 48, 3), 0.3, np.float32)
    for flags in (0, 1):
        for levels in (5, 10):
            out = D.denoise_cpu(ftn, rgb, gb, dict(levels=levels, flags=flags))
            assert np.abs(out / rgb - 1).max() <= 1e-6, (flags, levels)


@pytest.mark.parametrize("kind", ["normal", "coverage", "planes"])
def test_edges_keep_each_side(ftn, kind):
    """noise-free two-region images: the edge in the features keeps the two colours apart"""
    gb = R.gbuffer(40, 64, None, kind)
    right = np.arange(64)[None, :].repeat(40, 0) >= 32
    rgb = np.where(right[..., None], np.float32([0.05, 0.04, 0.06]), np.float32([0.4, 0.5, 0.3])).astype(np.float32)
    for flags in (0, 1):
        out = D.denoise_cpu(ftn, rgb, gb, dict(flags=flags))
        assert np.abs(out / rgb - 1).max() <= 1e-5, (kind, flags, np.abs(out / rgb - 1).max())


def test_demodulation_carries_an_albedo_edge(ftn):
    """one plane, constant irradiance, an albedo step: demodulated, the image is a fixed point; filtered as colour it is not"""
    gb = R.gbuffer(40, 64, None, "albedo")
    rgb = (gb[..., 0:3] * np.float32(0.7)).astype(np.float32)
    out = D.denoise_cpu(ftn, rgb, gb)
    assert np.abs(out / rgb - 1).max() <= 1e-5
    plain = D.denoise_cpu(ftn, rgb, gb, dict(flags=0))
    assert np.abs(plain / rgb - 1).max() > 1e-2                   # without demodulation the colour edge alone stops the filter less


def test_noise_is_reduced(ftn):
    """the mean of 4 gamma(0.25) samples per channel (about 4 spp of path tracing) over the mixed edge image"""
    rgb, gb, clean = R.synthetic(120, 200, seed=11)
    noisy = float(((rgb.astype(np.float64) - clean) ** 2).mean())
    out = D.denoise_cpu(ftn, rgb, gb)
    ratio = float(((out.astype(np.float64) - clean) ** 2).mean()) / noisy
    assert ratio <= 0.2, ratio
    for region in (gb[..., 10] == 0, (gb[..., 10] > 0) & (gb[..., 9] < 1.5)):       # region means stay within the noise
        assert abs(out[region].mean() / clean[region].mean() - 1) < 0.05


def test_result_does_not_depend_on_the_thread_count(ftn):
    rgb, gb, _ = R.synthetic(640, 640, seed=3)                     # 409,600 pixels: parallel_for uses up to 7 threads
    old = os.environ.get("FTN_BVH_THREADS")
    got = {}
    try:
        for nt in (1, 7):
            os.environ["FTN_BVH_THREADS"] = str(nt)
            got[nt] = D.denoise_cpu(ftn, rgb, gb, dict(levels=3))
    finally:
        if old is None: os.environ.pop("FTN_BVH_THREADS", None)
        else: os.environ["FTN_BVH_THREADS"] = old
    assert np.array_equal(bits(got[1]), bits(got[7]))


def test_non_finite_inputs(ftn):
    """a non-finite pixel is copied through (and remodulated); its neighbours ignore it; non-finite features weigh 0"""
    rgb, gb, _ = R.synthetic(48, 64, seed=21)
    rgb[10, 10] = (np.nan, 0.2, 0.3)
    rgb[20, 30] = (np.inf, 1.0, 1.0)
    rgb[30, 5] = (0.1, -np.inf, 0.1)
    rgb[40, 60] = np.nan                                            # (in the environment region of the mixed image)
    gb[5, 40, 3] = np.nan                                           # a non-finite normal
    gb[25, 20, 6] = np.inf                                          # a non-finite position
    for flags in (0, 1):
        out = D.denoise_cpu(ftn, rgb, gb, dict(flags=flags))
        want = R.reference(rgb, gb, flags=flags)
        assert_close(out, want)
        assert np.isnan(out[10, 10, 0]) and np.isnan(out[40, 60]).all() and out[20, 30, 0] == np.inf and out[30, 5, 1] == -np.inf
        bad = ~np.isfinite(rgb).all(-1)
        assert np.isfinite(out[~bad]).all()
        assert np.array_equal(bits(out[10, 10, 1:]), bits(D.denoise_cpu(ftn, rgb, gb, dict(flags=flags, levels=1))[10, 10, 1:]))


@pytest.mark.parametrize("t_target,above", [(95.0, False), (104.0, False), (104.0, True)])
def test_subnormal_weights_on_the_twin(ftn, t_target, above):
    """one tap whose weight exp(-t) is a binary32 subnormal (t about 95), the last t the filter keeps (104) and the first it drops: the
    black centre pixel takes exactly the header's binary32 value, a subnormal for t = 95 that flushing denormals would zero"""
    rgb, gb, p, t, want = R.one_tap(t_target, above)
    assert (t > 104.0) == above and abs(t - t_target) < 1e-3 * t_target
    got = D.denoise_cpu(ftn, rgb, gb, p)
    assert np.array_equal(bits(got[0, 2]), bits(np.full(3, want, np.float32)))
    if t_target < 100:
        assert 0 < want < np.finfo(np.float32).tiny
    ref, err = R.reference_bound(rgb, gb, **p)
    assert (np.abs(got - ref) <= err).all()
