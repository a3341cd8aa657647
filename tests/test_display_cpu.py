"""The display stage's host twins (include/fountain_hip_display.h) without a GPU, against the independent restatement of
tests/_display_ref.py: the histogram bit for bit, the exposure within one binary32 ulp of float64, the binary32 encode against float64
(codes differ by at most 1 and only on pixels whose float64 value lies within a measured delta of a rounding boundary), the curves'
monotony, black, white and the dither's mean, the special values, the PNG files through an independent reader, and the thread count.

Measured on the twin (2^20 pixels log-uniform in [2^-12, 2^6], the four curves under sRGB): the largest |v32 - v64| * 255 is 3.8e-5
(linear), 6.3e-5 (Reinhard), 6.4e-5 (ACES) and 6.6e-5 codes (Hable), so delta = 4 x 6.6e-5 = 2.64e-4 codes; the share of fragile pixels
(some channel within delta of an integer boundary) is 0.10 %, 0.12 %, 0.13 % and 0.15 % against the 0.5 % allowed, and 5, 3, 9 and 38 of
the 2^20 pixels differ by one code, every one of them fragile."""
import numpy as np
import pytest

from fountain_amd import _abi as A
from fountain_amd import display as D

import _display_ref as R

F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)


@pytest.fixture(scope="module")
def imgs():
    return R.images()


# ------------------------------------------------------------------ histogram
def test_histogram_against_numpy(ftn, imgs):
    for name, img in imgs.items():
        got, want = D.histogram_cpu(ftn, img), R.histogram(img)
        assert got.dtype == np.uint32 and got.shape == (A.FTN_DISPLAY_HIST_WORDS,)
        assert np.array_equal(got, want), name
        assert int(got.sum()) == img.shape[0] * img.shape[1] and got[387] == 0
    assert D.histogram_cpu(ftn, imgs["constant 512x512"]).max() == 262144          # more than a 16-bit counter holds
    assert np.count_nonzero(D.histogram_cpu(ftn, imgs["checker 48x64"])) == 2
    assert all(D.histogram_cpu(ftn, imgs["random 257x255"])[k] > 0 for k in (R.BELOW, R.ABOVE))


def test_every_salt_value_lands_in_the_counter_the_header_names(ftn):
    for name, value, word in R.SALT:
        px = R.salt_pixel(value).reshape(1, 1, 3)
        Y = R.luminance32(px)[0, 0]
        assert np.isnan(Y) if np.isnan(value) else (Y < 0 and np.isfinite(Y)) if value == -1 else Y == value, name
        got = D.histogram_cpu(ftn, px)
        assert got[word] == 1 and got.sum() == 1, (name, np.nonzero(got)[0])


def test_bins_from_bits_agree_with_the_logarithm(ftn):
    """the library takes the bin from the float's bits; the restatement here takes it from log2"""
    rng = np.random.default_rng(5)
    values = list(R.log_uniform(rng, 64, -24.0, 24.0))
    for edge in (0.25, 0.28125, 1.0, 1.875, 2.0 ** -24, 2.0 ** 23 * 1.875):
        values += [F32(edge), np.nextafter(F32(edge), F32(np.inf))] + ([np.nextafter(F32(edge), F32(0.0))] if edge > 2.0 ** -24 else [])
    for v in values:
        px = R.pixel_with_luminance(v, rng).reshape(1, 1, 3)
        assert np.nonzero(D.histogram_cpu(ftn, px))[0].tolist() == [R.bin_of(F32(v))], v
    assert R.bin_of(F32(0.25)) == R.bin_of(np.nextafter(F32(0.25), F32(0.0))) + 1 == 8 * 22


# ------------------------------------------------------------------ exposure
def _ulp_close(got, want64):
    w = F32(want64)
    return abs(float(got) - float(w)) <= float(np.spacing(w))


def test_exposure_against_float64(ftn, imgs):
    for name, img in imgs.items():
        hist = R.histogram(img)
        for kw in (dict(), dict(key=0.5, p_lo=0.0, p_hi=1.0), dict(p_lo=0.45, p_hi=0.55), dict(min_ev=-2.0, max_ev=3.0)):
            info = D.exposure(ftn, hist, dict(auto_exposure=True, **kw))
            scale, avg, empty = R.exposure64(hist, **kw)
            assert _ulp_close(info["scale"], scale), (name, kw, info, scale)
            assert abs(info["avg_log2"] - avg) <= 1e-12 * max(1.0, abs(avg)), (name, kw)
            assert info["flags"] == (A.FTN_DISPLAY_INFO_EMPTY if empty else 0)
            assert (info["count_bins"], info["count_invalid"], info["count_below"], info["count_above"]) == \
                (int(hist[:R.BINS].sum()), hist[R.INVALID], hist[R.BELOW], hist[R.ABOVE])
    for ev in (0.0, 1.0, -3.5, 2.25):
        info = D.exposure(ftn, None, dict(ev=ev))
        assert _ulp_close(info["scale"], 2.0 ** ev) and info["avg_log2"] == 0.0 and info["flags"] == 0


def test_exposure_edges(ftn):
    # nothing in the bins: scale 1 and the flag
    for img in (np.zeros((4, 4, 3), F32), np.full((4, 4, 3), NAN), np.full((4, 4, 3), INF)):
        info = D.exposure(ftn, D.histogram_cpu(ftn, img), dict(auto_exposure=True))
        assert info["scale"] == 1.0 and info["flags"] == A.FTN_DISPLAY_INFO_EMPTY and info["avg_log2"] == 0.0 and info["count_bins"] == 0
    # both clamps
    dark, bright = np.tile(R.pixel_with_luminance(2.0 ** -22), (8, 8, 1)), np.tile(R.pixel_with_luminance(2.0 ** 22), (8, 8, 1))
    assert D.exposure(ftn, D.histogram_cpu(ftn, dark), dict(auto_exposure=True))["scale"] == 2.0 ** 16
    assert D.exposure(ftn, D.histogram_cpu(ftn, bright), dict(auto_exposure=True))["scale"] == 2.0 ** -16
    assert D.exposure(ftn, D.histogram_cpu(ftn, bright), dict(auto_exposure=True, min_ev=3.0, max_ev=3.0))["scale"] == 8.0
    # a constant image at a bin's lower edge: every pixel in bin (o, m) = (-2, 0), so avg_log2 = -2 + log2(1 + 0.5 / 8)
    px = R.pixel_with_luminance(0.25)
    assert R.luminance32(px) == F32(0.25)
    info = D.exposure(ftn, D.histogram_cpu(ftn, np.tile(px, (16, 16, 1))), dict(auto_exposure=True))
    want = -2.0 + np.log2(1.0 + 0.5 / 8.0)
    assert abs(info["avg_log2"] - want) <= 1e-12 and _ulp_close(info["scale"], float(F32(0.18)) / 2.0 ** want) and info["count_bins"] == 256
    # just below the edge it is the bin before
    below = R.pixel_with_luminance(np.nextafter(F32(0.25), F32(0.0)))
    info = D.exposure(ftn, D.histogram_cpu(ftn, np.tile(below, (16, 16, 1))), dict(auto_exposure=True))
    assert abs(info["avg_log2"] - (-3.0 + np.log2(1.0 + 7.5 / 8.0))) <= 1e-12


# ------------------------------------------------------------------ encode against float64
CASES = [(tm, "srgb") for tm in R.TONEMAPS]


@pytest.fixture(scope="module")
def big(ftn):
    """2^20 pixels log-uniform in [2^-12, 2^6]; per case the twin's codes and float image and the float64 image; delta in codes"""
    rgb = R.log_uniform(np.random.default_rng(11), (1024, 1024, 3))
    out, worst = {}, 0.0
    for tm, tf in CASES:
        o8, of = D.encode_cpu(ftn, rgb, 1.0, dict(tonemap=tm, transfer=tf), want_float=True)
        v64 = R.display64(rgb, 1.0, tm, tf)
        err = float(np.abs(of.astype(np.float64) - v64).max()) * 255.0
        print("%s/%s: largest |v32 - v64| * 255 = %.3g codes" % (tm, tf, err))
        worst = max(worst, err)
        out[(tm, tf)] = (o8, of, v64)
    print("delta = 4 x %.3g = %.3g codes" % (worst, 4.0 * worst))
    return rgb, out, 4.0 * worst


@pytest.mark.parametrize("tm,tf", CASES)
def test_codes_against_float64(big, tm, tf):
    rgb, out, delta = big
    o8, of, v64 = out[(tm, tf)]
    assert 0.0 < delta < 1e-2                                               # a sanity bound on the measurement itself, far above binary32's error
    codes, alpha = R.unpack(o8)
    want, q = R.quantise64(v64)
    assert (alpha == 255).all()
    diff = np.abs(codes - want)
    fragile = (np.abs(q - np.rint(q)) < delta).any(axis=-1)
    share = float(fragile.mean())
    print("%s/%s: %d pixels differ by one code, fragile share %.4f %%" % (tm, tf, int((diff > 0).any(axis=-1).sum()), 100.0 * share))
    assert diff.max() <= 1
    assert not ((diff > 0).any(axis=-1) & ~fragile).any()
    assert share <= 0.005
    assert np.abs(of.astype(np.float64) - v64).max() <= delta / 255.0
    assert 0.0 <= of.min() and of.max() <= 1.0


@pytest.mark.parametrize("tf", ["gamma", "linear"])
@pytest.mark.parametrize("tm", R.TONEMAPS)
def test_codes_under_the_other_transfers(ftn, big, tm, tf):
    """the other transfers on the same pixels: no code further than 1 from float64's.  (Their delta is not the sRGB one: a pure power
    law has no linear toe, and below 1e-3 it multiplies the curves' binary32 error, Hable's difference of two near-equal quotients
    most of all, by up to 40.)"""
    rgb = big[0][:256]
    codes, alpha = R.unpack(D.encode_cpu(ftn, rgb, 1.0, dict(tonemap=tm, transfer=tf)))
    want, _ = R.quantise64(R.display64(rgb, 1.0, tm, tf))
    assert np.abs(codes - want).max() <= 1 and (alpha == 255).all()
    assert ((codes != want).any(axis=-1)).mean() <= 0.005


@pytest.mark.parametrize("tm", R.TONEMAPS)
@pytest.mark.parametrize("tf", R.TRANSFERS)
def test_monotone_on_a_grey_ramp(ftn, tm, tf):
    ramp = np.repeat(np.linspace(0.0, 16.0, 4096, dtype=np.float64).astype(F32)[None, :, None], 3, axis=-1)
    o8, of = D.encode_cpu(ftn, ramp, 1.0, dict(tonemap=tm, transfer=tf), want_float=True)
    codes, _ = R.unpack(o8)
    assert (np.diff(of[0], axis=0) >= 0).all() and (np.diff(codes[0], axis=0) >= 0).all()
    assert codes[0, 0].tolist() == [0, 0, 0] and codes[0, -1].tolist() == [255, 255, 255]
    assert len(np.unique(codes[0, :, 0])) > 128                                # the ramp is not flattened (its steps are coarse at the dark end)
    want, _ = R.quantise64(R.display64(ramp, 1.0, tm, tf))
    assert np.abs(codes - want).max() <= 1


@pytest.mark.parametrize("dither", [False, True])
def test_black_and_white_survive(ftn, dither):
    black, white = np.zeros((16, 24, 3), F32), np.full((16, 24, 3), 1.0e4, F32)
    for tm in R.TONEMAPS:
        for tf in R.TRANSFERS:
            p = dict(tonemap=tm, transfer=tf, dither=dither)
            assert (D.encode_cpu(ftn, black, 1.0, p) == 0xff000000).all(), p
            assert (D.encode_cpu(ftn, white, 1.0, p) == 0xffffffff).all(), p
    assert (D.encode_cpu(ftn, np.full((16, 24, 3), 1.0, F32), 1.0, dict(tonemap="linear", transfer="linear", dither=dither)) == 0xffffffff).all()


def test_dither(ftn):
    """an ordered dither's guarantee: over any aligned 8 x 8 block of a constant grey v the mean code is within 1/64 of v * 255"""
    p = dict(tonemap="linear", transfer="linear", dither=True)
    for v in (0.0, 0.001, 0.1234, 0.5, 100.3 / 255.0, 100.5 / 255.0, 100.99 / 255.0, 0.9990, 1.0):
        img = np.full((16, 24, 3), v, F32)
        codes, _ = R.unpack(D.encode_cpu(ftn, img, 1.0, p))
        for y0 in (0, 8):
            for x0 in (0, 8, 16):
                block = codes[y0:y0 + 8, x0:x0 + 8, 0]
                assert abs(block.mean() - float(F32(v)) * 255.0) <= 1.0 / 64.0, v
                assert block.max() - block.min() <= 1
        assert np.array_equal(codes[..., 0], codes[..., 1]) and np.array_equal(codes[..., 0], codes[..., 2])
    # each pixel takes the matrix entry of its own (x & 7, y & 7): against the restatement's table, on sizes that are no multiple of 4 or 8
    rng = np.random.default_rng(3)
    for h, w in ((1, 1), (1, 3), (3, 1), (7, 5), (53, 37)):
        img = rng.uniform(0.0, 1.0, (h, w, 3)).astype(F32)
        codes, _ = R.unpack(D.encode_cpu(ftn, img, 1.0, p))
        want, q = R.quantise64(R.display64(img, 1.0, "linear", "linear"), dither=True)
        safe = (np.abs(q - np.rint(q)) > 1e-3)
        assert np.array_equal(codes[safe], want[safe]) and safe.mean() > 0.99


def test_special_values(ftn):
    rows = [[NAN, 0.5, 0.5], [0.5, NAN, NAN], [INF, 0.0, 0.0], [INF, INF, INF], [-INF, 0.5, 0.25], [-1.0, -2.0, -3.0], [-0.0, 0.0, 1e-40],
            [65504.0, 1e30, 3e38], [NAN, INF, -INF]]
    img = np.array(rows, F32).reshape(3, 3, 3)
    for tm in R.TONEMAPS:
        for tf in R.TRANSFERS:
            for scale in (1.0, 0.0, 1e-3, 1e30):
                o8, of = D.encode_cpu(ftn, img, scale, dict(tonemap=tm, transfer=tf), want_float=True)
                assert np.isfinite(of).all() and of.min() >= 0.0 and of.max() <= 1.0
                v64 = R.display64(img, scale, tm, tf)
                want, q = R.quantise64(v64)
                codes, alpha = R.unpack(o8)
                assert np.abs(codes - want).max() <= 1 and (alpha == 255).all(), (tm, tf, scale)
    # what the header says: NaN, negatives and -inf are 0; +inf is the largest value and saturates
    codes, _ = R.unpack(D.encode_cpu(ftn, img, 1.0, dict(tonemap="aces")))
    flat = codes.reshape(9, 3)
    assert flat[0, 0] == 0 and flat[1, 1] == 0 and flat[1, 2] == 0 and flat[4, 0] == 0 and flat[5].tolist() == [0, 0, 0] and flat[6].tolist() == [0, 0, 0]
    assert flat[2].tolist() == [255, 0, 0] and flat[3].tolist() == [255, 255, 255] and flat[8].tolist() == [0, 255, 0]


def test_linear_linear_is_a_clamp(ftn, imgs):
    for name in ("random 37x53", "salted 37x53", "random 257x255"):
        img = imgs[name]
        _, of = D.encode_cpu(ftn, img, D.exposure(ftn, None, dict(ev=0.0))["scale"], dict(tonemap="linear", transfer="linear"), want_float=True)
        with np.errstate(invalid="ignore"):
            want = np.where(img > 0, np.minimum(img, F32(1.0)), F32(0.0)).astype(F32)
        assert np.array_equal(of.view(np.uint32), want.view(np.uint32)), name


def test_srgb_knee(ftn):
    """v <= 0.0031308f takes the linear segment, the knee itself included: there the two segments differ by 7 binary32 ulps"""
    knee = F32(0.0031308)
    above, below = np.nextafter(knee, F32(1.0)), np.nextafter(knee, F32(0.0))
    img = np.array([[[knee, above, below]]], F32)
    _, of = D.encode_cpu(ftn, img, 1.0, dict(tonemap="linear"), want_float=True)
    assert of[0, 0, 0] == F32(12.92) * knee and of[0, 0, 2] == F32(12.92) * below
    power = 1.055 * float(above) ** (1.0 / 2.4) - 0.055
    assert of[0, 0, 1] != F32(12.92) * above and abs(float(of[0, 0, 1]) - power) <= 2.0 * float(np.spacing(F32(power)))
    assert abs(float(F32(12.92) * knee) - (1.055 * float(knee) ** (1.0 / 2.4) - 0.055)) > 4.0 * float(np.spacing(F32(0.04045)))


def test_chain_and_shared_exposure(ftn, imgs):
    img = imgs["random 37x53"]
    p = dict(auto_exposure=True, tonemap="reinhard")
    o8, of, info = D.display_cpu(ftn, img, p, want_float=True)
    scale, _, _ = R.exposure64(R.histogram(img))
    assert _ulp_close(info["scale"], scale)
    again = D.encode_cpu(ftn, img, info["scale"], p)
    assert np.array_equal(o8, again)
    # the automatic-mode fields and ev are not read by the encode
    assert np.array_equal(o8, D.encode_cpu(ftn, img, info["scale"], dict(tonemap="reinhard", ev=5.0, key=0.9)))


# ------------------------------------------------------------------ PNG
@pytest.mark.parametrize("w,h", [(1, 1), (5, 7), (37, 53)])
def test_png(ftn, tmp_path, w, h):
    rng = np.random.default_rng(w)
    px = rng.integers(0, 2 ** 32, (h, w), dtype=np.uint64).astype(np.uint32)         # the alpha byte is anything: it is dropped
    rgb = np.stack([(px >> s) & 0xff for s in (0, 8, 16)], axis=-1).astype(np.uint8)
    for gamma, chunk in ((None, "sRGB"), (2.2, "gAMA"), (1.0, "gAMA")):
        path = str(tmp_path / ("g%s.png" % gamma))
        D.write_png(path, px, ftn, gamma)
        png = R.read_png(path)                                                       # checks the signature and every CRC
        assert png["chunks"] == ["IHDR", chunk, "IDAT", "IEND"]
        assert (png["width"], png["height"], png["bit_depth"], png["colour_type"], png["compression"], png["filter_method"], png["interlace"]) == \
            (w, h, 8, 2, 0, 0, 0)
        assert (png["srgb_intent"], png["gama"]) == ((0, None) if gamma is None else (None, {2.2: 45455, 1.0: 100000}[gamma]))
        assert (png["filters"] == 0).all() and len(png["filters"]) == h
        assert np.array_equal(png["pixels"], rgb)


def test_png_unwritable_path(ftn, tmp_path):
    from fountain_amd import FountainError
    with pytest.raises(FountainError) as e:
        D.write_png(str(tmp_path / "missing" / "a.png"), np.zeros((2, 2), np.uint32), ftn)
    assert e.value.code == A.FTN_ERR_INVALID_ARGUMENT and "cannot create" in str(e.value)
    assert not list(tmp_path.iterdir())


# ------------------------------------------------------------------ threads
def test_thread_count_changes_no_bit(ftn, big, imgs, monkeypatch):
    rgb, out, _ = big
    monkeypatch.setenv("FTN_BVH_THREADS", "1")
    one = (D.histogram_cpu(ftn, rgb), D.encode_cpu(ftn, rgb, 0.7, dict(dither=True), want_float=True), D.histogram_cpu(ftn, imgs["salted 37x53"]))
    assert D.histogram_cpu(ftn, imgs["constant 512x512"]).max() == 262144      # one thread counts all of them: no 16-bit counter anywhere
    for threads in ("3", "7"):
        monkeypatch.setenv("FTN_BVH_THREADS", threads)
        more = (D.histogram_cpu(ftn, rgb), D.encode_cpu(ftn, rgb, 0.7, dict(dither=True), want_float=True), D.histogram_cpu(ftn, imgs["salted 37x53"]))
        assert np.array_equal(one[0], more[0]) and np.array_equal(one[2], more[2])
        assert np.array_equal(one[1][0], more[1][0]) and np.array_equal(one[1][1].view(np.uint32), more[1][1].view(np.uint32))
    monkeypatch.delenv("FTN_BVH_THREADS")
    assert np.array_equal(one[0], R.histogram(rgb))
