"""The host twin of the measuring stage (ftn_metrics_cpu, include/fountain_hip_metrics.h) without a GPU, against tests/_metrics_ref.py:
bit equality with the float64 restatement on every size the GPU tests use; an independent SSIM in another summation order; the exact
properties the specification promises; the command line."""
import json
import math
import os

import numpy as np
import pytest

from fountain_amd import metrics as M

import _metrics_ref as R

F32, F64 = np.float32, np.float64
SIZES = [(1, 1), (5, 33), (11, 11), (12, 11), (16, 16), (17, 16), (16, 17), (48, 16), (80, 16), (27, 43), (272, 272)]       # (w, h)
ALL = dict(error_map=True, tile_sums=True, totals=True)
bits32, bits64 = R.bits32, R.bits64


def same_bits(got, want, keys):
    for k in keys:
        assert np.array_equal(bits64(got[k]), bits64(want[k])), (k, got[k], want[k])


RESULT_F64 = ("mse", "rmse", "mae", "rel_mse", "smape", "ssim", "mse_rgb", "max_abs")
RESULT_INT = ("max_abs_index", "n_pixels", "n", "n_nonfinite", "n_different", "n_ssim_windows")


def check_against_restatement(got, want, ssim):
    assert np.array_equal(bits64(got["tile_sums"]), bits64(want["tile_sums"]))
    same_bits(got["totals"], want["totals"], ("sum", "max_abs"))
    for k in ("max_abs_index", "n_pixels", "n_nonfinite", "n_different", "n_ssim_windows"):
        assert got["totals"][k] == want["totals"][k], k
    same_bits(got, want["result"], RESULT_F64)
    for k in RESULT_INT:
        assert got[k] == want["result"][k], k
    # log10 is the host's on both sides, but no libm promises the last bit of it
    assert got["psnr"] == want["result"]["psnr"] or abs(got["psnr"] - want["result"]["psnr"]) <= 4e-16 * abs(got["psnr"])
    assert np.array_equal(bits32(got["error_map"]), bits32(want["error_map"]))
    if ssim:
        assert np.array_equal(bits32(got["ssim_map"]), bits32(want["ssim_map"]))


# ------------------------------------------------------------------ 1. the twin equals the restatement, bit for bit
@pytest.mark.parametrize("scale", [1.0, 100.0], ids=["unit", "hdr"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_twin_equals_the_restatement(ftn, size, scale):
    w, h = size
    test, ref = R.images(w, h, scale=scale)
    g = M.ssim_weights(ftn)
    for ssim in (False, True) if min(w, h) >= 11 else (False,):
        for peak in (1.0, scale):
            got = M.compare_cpu(ftn, test, ref, dict(ssim=ssim, peak=peak), ssim_map=ssim, **ALL)
            check_against_restatement(got, R.reference(test, ref, peak=peak, ssim=ssim, g=g), ssim)
    got = M.compare_cpu(ftn, test, ref, dict(rel_eps=1e-4), **ALL)
    check_against_restatement(got, R.reference(test, ref, rel_eps=1e-4), False)
    assert math.isnan(got["ssim"]) and got["n_ssim_windows"] == 0 and not got["tile_sums"][:, 7].any()


def test_special_values(ftn):
    """signed zeros, subnormals, the largest finite values, equal pixels, and every kind of bad pixel"""
    w, h = 21, 19
    test, ref = R.images(w, h)
    test[0, 0] = (0.0, -0.0, 1e-45)
    ref[0, 0] = (-0.0, -0.0, 0.0)
    test[1, 1] = (3.4028235e38, -3.4028235e38, 1e-38)
    ref[1, 1] = (-3.4028235e38, -3.4028235e38, 3.4028235e38)
    test[2:5] = ref[2:5]
    test[7, 3, 1] = np.nan
    ref[8, 20, 2] = np.inf
    test[18, 0, 0] = -np.inf
    ref[18, 0, 0] = -np.inf
    test[9, 9] = ref[9, 9] = np.array([0x7fc12345, 0x3f800000, 0x3f800000], np.uint32).view(F32)     # the same NaN on both sides: bad, not different
    g = M.ssim_weights(ftn)
    got = M.compare_cpu(ftn, test, ref, dict(ssim=True), ssim_map=True, **ALL)
    check_against_restatement(got, R.reference(test, ref, ssim=True, g=g), True)
    assert got["n_nonfinite"] == 4 and got["max_abs"] == 2.0 * 3.4028234663852886e38 and got["max_abs_index"] == w + 1
    assert got["n_different"] == w * h - 3 * w - 1                       # three equal rows, and (9, 9) carries the same bits on both sides


# ------------------------------------------------------------------ 2. an independent SSIM
def _independent_inputs():
    rng = np.random.default_rng(7)
    shape = (43, 27, 3)
    out = []
    for name, scale, peak in (("unit", 1.0, 1.0), ("hdr100", 100.0, 1.0), ("hdr100_peak100", 100.0, 100.0)):
        a = (scale * rng.random(shape)).astype(F32)
        out.append((name, a, (a + 0.1 * scale * rng.standard_normal(shape)).astype(F32), peak))
    out.append(("ill_conditioned", (0.9 + 1e-3 * rng.random(shape)).astype(F32), (0.9 + 1e-3 * rng.random(shape)).astype(F32), 1.0))
    return out


@pytest.mark.parametrize("case", _independent_inputs(), ids=lambda c: c[0])
def test_ssim_against_another_summation_order(ftn, case):
    """scipy's 2-D correlation with the 11 x 11 outer-product kernel sums a window's 121 products in one pass; the specification sums 11
    and then 11.  Measured on 43 x 27 inputs before the code existed: at most 6.6e-15 per pixel on random inputs, 2.3e-12 on the
    ill-conditioned one (a constant 0.9 with a 1e-3 texture: the variances cancel 6 digits), so 1e-10 is 40 times the worst."""
    name, test, ref, peak = case
    g = M.ssim_weights(ftn)
    got = M.compare_cpu(ftn, test, ref, dict(ssim=True, peak=peak), ssim_map=True, **ALL)
    mine = R.reference(test, ref, peak=peak, ssim=True, g=g)
    check_against_restatement(got, mine, True)                            # so the restatement's binary64 pixels below are the twin's
    other = R.reference(test, ref, peak=peak, ssim=True, g=g, moments=R.independent_moments)
    win = R.windows(R.bad_pixels(test, ref))
    assert win.sum() == 33 * 17 == got["n_ssim_windows"]
    per_pixel = np.abs(mine["ssim_pixels"][win] - other["ssim_pixels"][win]) / 3.0
    mean = float(other["ssim_pixels"][win].mean() / 3.0)
    print("independent SSIM, %s: largest per-pixel difference %.3g, mean %.17g against %.17g (difference %.3g)"
          % (name, per_pixel.max(), got["ssim"], mean, abs(got["ssim"] - mean)))
    assert per_pixel.max() <= 1e-10
    assert abs(got["ssim"] - mean) <= 1e-10
    # the binary32 map within one binary32 ulp of the independent one, NaN in the same places
    a, b = got["ssim_map"], other["ssim_map"]
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isnan(a), ~win)
    assert (np.abs(a[win].astype(F64) - b[win].astype(F64)) <= np.spacing(np.abs(b[win]))).all()


# ------------------------------------------------------------------ 3. exact properties
@pytest.mark.parametrize("case", _independent_inputs(), ids=lambda c: c[0])
def test_an_image_against_itself(ftn, case):
    _, x, _, peak = case
    r = M.compare_cpu(ftn, x, x, dict(ssim=True, peak=peak), ssim_map=True, **ALL)
    for k in ("mse", "rmse", "mae", "rel_mse", "smape", "max_abs"):
        assert r[k] == 0.0 and not math.copysign(1.0, r[k]) < 0, k
    assert r["mse_rgb"] == (0.0, 0.0, 0.0) and r["psnr"] == math.inf and r["n_different"] == 0 and r["max_abs_index"] == 0
    win = R.windows(R.bad_pixels(x, x))
    assert (r["ssim_map"][win] == 1.0).all() and r["ssim"] == 1.0         # every ssim_c is exactly 1, so the sums are exact
    assert np.array_equal(bits64(r["tile_sums"][:, 7]), bits64(R.tile_sums(3.0 * win)))
    assert not r["error_map"].any()
    # the same buffer and an equal copy are the same thing
    again = M.compare_cpu(ftn, x, x.copy(), dict(ssim=True, peak=peak), ssim_map=True, **ALL)
    assert np.array_equal(bits64(again["tile_sums"]), bits64(r["tile_sums"])) and again["totals"] == r["totals"]


def test_constant_images_give_the_closed_forms(ftn):
    w, h = 37, 21
    test, ref = np.full((h, w, 3), 0.75, F32), np.full((h, w, 3), 0.5, F32)
    r = M.compare_cpu(ftn, test, ref, dict(ssim=True), **ALL)
    assert r["mse"] == 0.0625 and r["rmse"] == 0.25 and r["mae"] == 0.25 and r["max_abs"] == 0.25 and r["max_abs_index"] == 0
    assert r["mse_rgb"] == (0.0625, 0.0625, 0.0625) and r["n_different"] == w * h and r["n"] == w * h
    assert abs(r["psnr"] - 10.0 * math.log10(16.0)) <= 1e-14
    assert r["totals"]["sum"][0] == 0.1875 * w * h and r["totals"]["sum"][1] == 0.75 * w * h
    eps = float(F32(1e-2))
    assert abs(r["rel_mse"] - 0.0625 / (0.25 + eps)) <= 1e-15 and abs(r["smape"] - 0.25 / (1.25 + eps)) <= 1e-15
    # a tile's sum is its pixel count times the pixel's term: the clipped tiles at the right and the bottom too
    counts = R.tile_sums(np.ones((h, w)))
    assert np.array_equal(r["tile_sums"][:, 0], 0.1875 * counts) and sorted(set(counts)) == [5 * 5, 5 * 16, 16 * 16]
    assert np.array_equal(r["error_map"], np.full((h, w), 0.0625, F32))


def test_swapping_test_and_ref(ftn):
    test, ref = R.images(43, 27, scale=3.0)
    p = dict(ssim=True, peak=3.0)
    a, b = M.compare_cpu(ftn, test, ref, p, ssim_map=True, **ALL), M.compare_cpu(ftn, ref, test, p, ssim_map=True, **ALL)
    same_bits(a, b, ("mse", "rmse", "mae", "smape", "ssim", "psnr", "mse_rgb", "max_abs"))
    assert a["n_different"] == b["n_different"] and a["max_abs_index"] == b["max_abs_index"]
    assert np.array_equal(bits32(a["ssim_map"]), bits32(b["ssim_map"])) and np.array_equal(bits32(a["error_map"]), bits32(b["error_map"]))
    assert a["rel_mse"] != b["rel_mse"]


def test_one_nan_pixel(ftn):
    w, h, x0, y0 = 43, 37, 20, 17
    test, ref = R.images(w, h)
    clean = M.compare_cpu(ftn, test, ref, dict(ssim=True), ssim_map=True, **ALL)
    bad = test.copy()
    bad[y0, x0, 1] = np.nan
    r = M.compare_cpu(ftn, bad, ref, dict(ssim=True), ssim_map=True, **ALL)
    assert r["n_nonfinite"] == 1 and r["n"] == w * h - 1 and r["n_different"] == clean["n_different"]
    # exactly the windows that touch it are missing
    gone = np.isnan(r["ssim_map"]) & ~np.isnan(clean["ssim_map"])
    want = np.zeros((h, w), bool)
    want[y0 - 5:y0 + 6, x0 - 5:x0 + 6] = True
    assert np.array_equal(gone, want) and r["n_ssim_windows"] == clean["n_ssim_windows"] - 121
    assert np.array_equal(bits32(r["ssim_map"])[~want], bits32(clean["ssim_map"])[~want])
    # the pointwise sums are those of the image with that pixel's terms zeroed: a pixel equal on both sides has all-zero terms
    zeroed = test.copy()
    zeroed[y0, x0] = ref[y0, x0]
    z = M.compare_cpu(ftn, zeroed, ref, **ALL)
    assert np.array_equal(bits64(r["tile_sums"][:, :7]), bits64(z["tile_sums"][:, :7]))
    assert np.array_equal(bits64(r["totals"]["sum"][:7]), bits64(z["totals"]["sum"][:7]))
    assert np.isnan(r["error_map"][y0, x0]) and np.isnan(r["error_map"]).sum() == 1
    # the SSIM sum: the clean image's map with those windows zeroed, through the same tree
    g = M.ssim_weights(ftn)
    mine = R.reference(bad, ref, ssim=True, g=g)
    assert np.array_equal(bits64(r["tile_sums"]), bits64(mine["tile_sums"]))
    cleanref = R.reference(test, ref, ssim=True, g=g)
    assert np.array_equal(bits64(r["tile_sums"][:, 7]), bits64(R.tile_sums(np.where(want, 0.0, np.where(R.windows(np.zeros((h, w), bool)), cleanref["ssim_pixels"], 0.0)))))
    # every pixel bad: the means over nothing
    none = M.compare_cpu(ftn, np.full((12, 12, 3), np.nan, F32), np.zeros((12, 12, 3), F32), dict(ssim=True), ssim_map=True, **ALL)
    assert none["n"] == 0 and none["n_nonfinite"] == 144 and none["n_ssim_windows"] == 0 and none["n_different"] == 144
    assert all(math.isnan(none[k]) for k in ("mse", "rmse", "mae", "rel_mse", "smape", "psnr", "ssim", "max_abs")) and none["totals"]["max_abs"] == 0.0
    assert np.isnan(none["ssim_map"]).all() and np.isnan(none["error_map"]).all() and not none["tile_sums"].any()


def test_result_does_not_depend_on_the_thread_count(ftn):
    w, h = 800, 600                                                      # above the pixel count at which the host passes take eight threads
    test, ref = R.images(w, h)
    test[300, 400, 0] = np.inf
    got = {}
    old = os.environ.get("FTN_BVH_THREADS")
    try:
        for nt in (1, 8):
            os.environ["FTN_BVH_THREADS"] = str(nt)
            got[nt] = M.compare_cpu(ftn, test, ref, dict(ssim=True), ssim_map=True, **ALL)
    finally:
        if old is None: os.environ.pop("FTN_BVH_THREADS", None)
        else: os.environ["FTN_BVH_THREADS"] = old
    assert got[1]["totals"] == got[8]["totals"]
    assert np.array_equal(bits64(got[1]["tile_sums"]), bits64(got[8]["tile_sums"]))
    for k in ("error_map", "ssim_map"):
        assert np.array_equal(bits32(got[1][k]), bits32(got[8][k]))
    same_bits(got[1], got[8], RESULT_F64 + ("psnr",))
    assert got[1]["n_nonfinite"] == 1 and got[1]["n_ssim_windows"] == (w - 10) * (h - 10) - 121


# ------------------------------------------------------------------ 4. the command line
def test_cli(ftn, tmp_path, capsys):
    from fountain_amd.api import read_exr, write_exr
    w, h = 43, 27
    test, ref = R.images(w, h)
    a, b = str(tmp_path / "test.exr"), str(tmp_path / "ref.exr")
    write_exr(a, test, ftn)
    write_exr(b, ref, ftn)
    want = M.compare_cpu(ftn, test, ref, dict(ssim=True), ssim_map=True, **ALL)
    capsys.readouterr()
    assert M.main([a, b, "--cpu", "--ssim", "--json"]) == 0
    got = json.loads(capsys.readouterr().out)
    for k in RESULT_F64 + ("psnr",):
        assert np.array_equal(bits64(got[k]), bits64(want[k])), k
    for k in RESULT_INT:
        assert got[k] == want[k], k
    assert got["exceeded"] == [] and got["ssim_computed"] is True
    # the plain line
    assert M.main([a, b, "--cpu"]) == 0
    line = capsys.readouterr().out
    assert line.startswith("metrics: rmse %.6g " % want["rmse"]) and "ssim" not in line and "%d of %d pixels differ" % (w * h, w * h) in line
    # thresholds: 0 when every one holds, 1 when one is exceeded or NaN
    assert M.main([a, b, "--cpu", "--fail-above", "rmse=%r" % want["rmse"], "--fail-above", "max_abs=1e9"]) == 0
    assert M.main([a, b, "--cpu", "--fail-above", "rmse=%r" % float(np.nextafter(want["rmse"], 0.0)), "--fail-above", "max_abs=1e9"]) == 1
    assert M.main([a, a, "--cpu", "--fail-above", "rmse=0", "--fail-above", "n_different=0"]) == 0
    assert M.main([a, b, "--cpu", "--fail-above", "n_different=0"]) == 1
    nan = str(tmp_path / "nan.exr")
    write_exr(nan, np.full((h, w, 3), np.nan, F32), ftn)
    assert M.main([nan, b, "--cpu", "--fail-above", "rmse=1e30"]) == 1                                 # a mean over nothing is NaN, and NaN exceeds
    assert M.main([nan, b, "--cpu", "--fail-above", "n_nonfinite=%d" % (w * h)]) == 0
    assert M.main([a, b, "--cpu", "--json", "--fail-above", "mae=0"]) == 1
    assert json.loads(capsys.readouterr().out.splitlines()[-1])["exceeded"] == ["mae"]
    # the maps, read back
    e, s, t = (str(tmp_path / n) for n in ("e.exr", "s.exr", "t.exr"))
    assert M.main([a, b, "--cpu", "--ssim", "--error-map", e, "--ssim-map", s, "--tile-map", t, "--peak", "1", "--rel-eps", "0.01"]) == 0
    em, sm, tm = read_exr(e, ftn), read_exr(s, ftn), read_exr(t, ftn)
    for c in range(3):
        assert np.array_equal(bits32(em[..., c]), bits32(want["error_map"])) and np.array_equal(bits32(sm[..., c]), bits32(want["ssim_map"]))
    assert tm.shape == (2, 3, 3)
    counts = R.tile_sums(np.ones((h, w))).reshape(2, 3)
    assert np.array_equal(tm[..., 0], (want["tile_sums"][:, 0].reshape(2, 3) / (3.0 * counts)).astype(F32))
    # sizes that differ
    other = str(tmp_path / "other.exr")
    write_exr(other, np.zeros((w, h, 3), F32), ftn)
    before = sorted(f.name for f in tmp_path.iterdir())
    assert M.main([a, other, "--cpu", "--error-map", str(tmp_path / "x.exr")]) == 2
    assert sorted(f.name for f in tmp_path.iterdir()) == before
