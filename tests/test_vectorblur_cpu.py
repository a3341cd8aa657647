"""The vector-blur stage's host twin (ftn_vectorblur_cpu, ftn_vectorblur_velocities_cpu) without a GPU, against the numpy restatement
tests/_vectorblur_ref.py: the exact copies; a sharp static foreground; non-finite colours; steps 1 to 3 bit for bit (the clamp, the ties, one
fast pixel reaching exactly the 3 x 3 tiles around it); step 4 within a bound derived from the number of roundings; constants; the thread
count."""
import numpy as np
import pytest

from fountain_amd import vectorblur as V

import _vectorblur_ref as R

F32 = np.float32
bits = R.bits
EPS = 2.0 ** -23


def payloads(shape, seed=5):
    """an image whose bit patterns include NaNs with payloads, infinities, -0 and denormals"""
    rng = np.random.default_rng(seed)
    img = R.image(shape[1], shape[0], seed).reshape(-1)
    special = np.array([0x7fc12345, 0xffc00001, 0x7f800001, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x80000001], np.uint32).view(F32)
    at = rng.choice(img.size, size=min(img.size, 24), replace=False)
    img[at] = special[np.arange(at.size) % special.size]
    return img.reshape(shape[0], shape[1], 3)


# ------------------------------------------------------------------ exact copies
def test_exact_copies(ftn):
    w, h = 37, 21
    img = payloads((h, w))
    moving = R.field("uniform", w, h)
    cases = [("shutter 0", moving, dict(shutter=0.0)), ("no motion", np.zeros((h, w, 2), F32), {}), ("unknown motion", np.full((h, w, 2), np.nan, F32), {}),
             ("half a pixel at most", np.full((h, w, 2), F32(2.0)) * np.array([0.0, -1.0], F32), {})]         # |h| = 0.25 * 2 = 0.5
    for name, m, p in cases:
        for gb in (None, R.gbuffer(w, h)):
            got = V.vector_blur_cpu(ftn, img, m, gb, p)
            assert np.array_equal(bits(got), bits(img)), name
    assert float(V.velocities_cpu(ftn, cases[3][1])["neighbours"][..., 2].max()) <= 0.25
    one = payloads((1, 1))
    for taps in R.TAPS:
        assert np.array_equal(bits(V.vector_blur_cpu(ftn, one, np.full((1, 1, 2), 30.0, F32), None, dict(taps=taps))), bits(one))
    # a pixel and a half does blur (whole-pixel taps: a half velocity below one pixel reaches no tap with a weight above 0)
    m = np.full((h, w, 2), F32(6.0)) * np.array([1.0, 0.0], F32)
    assert not np.array_equal(bits(V.vector_blur_cpu(ftn, R.image(w, h), m)), bits(R.image(w, h)))


def test_sharp_foreground(ftn):
    """a static block nearer than the moving background by far more than the extent keeps its bits; the background around it blurs"""
    w, h = 48, 32
    img = R.image(w, h)
    m = np.zeros((h, w, 2), F32)
    m[...] = (40.0, 0.0)
    gb = np.zeros((h, w, 12), F32)
    gb[..., 9], gb[..., 10] = 10.0, 1.0
    block = (slice(10, 22), slice(14, 30))
    m[block] = 0.0
    gb[block + (9,)] = 2.0
    got = V.vector_blur_cpu(ftn, img, m, gb)
    assert np.array_equal(bits(got[block]), bits(img[block]))
    outside = np.ones((h, w), bool)
    outside[block] = False
    assert (bits(got) != bits(img)).any(-1)[outside].mean() > 0.9
    # without the G-buffer every pixel is at one depth and the background smears over the block's edge columns
    flat = V.vector_blur_cpu(ftn, img, m, None)
    assert (bits(flat[block]) != bits(img[block])).any()
    # the other way round: a background block (coverage 0) behind a moving foreground is blurred over
    gb2 = gb.copy()
    gb2[block + (10,)] = 0.0
    assert (bits(V.vector_blur_cpu(ftn, img, m, gb2)[block]) != bits(img[block])).any()


def test_non_finite_colour_stays_and_spreads_nowhere(ftn):
    w, h = 48, 32
    m = R.field("uniform", w, h)
    clean = R.image(w, h)
    img = clean.copy()
    bad = [(5, 7), (16, 16), (31, 47), (0, 0)]
    for k, (y, x) in enumerate(bad):
        img[y, x, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    got = V.vector_blur_cpu(ftn, img, m)
    assert np.isfinite(got).sum() == got.size - len(bad)
    for y, x in bad:
        assert np.array_equal(bits(got[y, x]), bits(img[y, x]))
    want, copied, peak = R.blur(img, m)
    ok = np.isfinite(img).all(-1)
    assert (np.abs(got[ok].astype(np.float64) - want[ok]).max(-1) <= (16 + 16) * EPS * peak[ok]).all()
    # and it differs from the clean image's blur exactly where a bad pixel would have been a tap
    differs = (bits(got) != bits(V.vector_blur_cpu(ftn, clean, m))).any(-1)
    assert differs.sum() > len(bad) and differs.sum() < 16 * len(bad) + len(bad)


# ------------------------------------------------------------------ steps 1 to 3, bit for bit
def same_records(ftn, m, gb=None, **p):
    got, want = V.velocities_cpu(ftn, m, gb, p), R.velocities(m, gb, **p)
    for k in ("pixels", "tiles", "neighbours"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    return got


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
def test_records_equal_the_restatement(ftn, size):
    w, h = size
    for name in R.FIELDS:
        for gb in (None, R.gbuffer(w, h)):
            for p in (dict(), dict(shutter=1.0, max_radius=3.5), dict(shutter=0.3, max_radius=16.0)):
                same_records(ftn, R.field(name, w, h), gb, **p)


def test_clamp_ties_and_reach(ftn):
    # the clamp: lengths at, just below and beyond max_radius; len is max_radius exactly where it clamps
    m = np.zeros((16, 16, 2), F32)
    m[0, :6, 0] = (8.0, 8.000001, 7.999999, 1e30, -3e38, 3e38)
    m[1, :3] = ((6.0, 8.0), (6.01, 8.0), (1e20, 1e20))                # the last one's len2 overflows: h = 0 with len = max_radius
    rec = same_records(ftn, m, None, shutter=1.0, max_radius=4.0)["pixels"]
    assert rec[0, 0, 2] == 4.0 and rec[0, 2, 2] < 4.0 and (rec[0, 3:6, 2] == 4.0).all() and rec[1, 0, 2] == 5.0 - 1.0
    assert (rec[1, 2, :3] == (0.0, 0.0, 4.0)).all() and (rec[..., 2] <= 4.0).all()
    # ties: equal lengths in several pixels of a tile and several tiles -> the smallest pixel index, then the smallest tile index
    w, h = 48, 48
    m = np.zeros((h, w, 2), F32)
    for y, x, v in ((20, 25, (12.0, 0.0)), (20, 21, (0.0, 12.0)), (17, 30, (0.0, -12.0)), (40, 40, (-12.0, 0.0)), (3, 40, (12.0, 0.0))):
        m[y, x] = v
    got = same_records(ftn, m)
    assert tuple(got["tiles"][1, 1][:3]) == (0.0, -3.0, 9.0)                  # (17, 30) has the smallest index of the middle tile's three
    assert tuple(got["tiles"][2, 2][:3]) == (-3.0, 0.0, 9.0) and tuple(got["tiles"][0, 2][:3]) == (3.0, 0.0, 9.0)
    assert tuple(got["neighbours"][1, 1][:3]) == (3.0, 0.0, 9.0)              # tile (0, 2) comes before (1, 1) and (2, 2)
    assert tuple(got["neighbours"][2, 0][:3]) == (0.0, -3.0, 9.0)             # only the middle tile is in reach
    # one fast pixel in a tile's corner reaches exactly the 3 x 3 tiles around it
    w, h = 80, 48
    m = np.zeros((h, w, 2), F32)
    m[16, 32] = (64.0, 64.0)                                                  # the first pixel of tile (1, 2); clamped to length 16
    got = same_records(ftn, m)
    reached = got["neighbours"][..., 2] > 0
    want = np.zeros((3, 5), bool)
    want[0:3, 1:4] = True
    assert np.array_equal(reached, want) and np.allclose(got["neighbours"][reached][:, 2], 256.0)
    img = R.image(w, h)
    out = V.vector_blur_cpu(ftn, img, m)
    changed = (bits(out) != bits(img)).any(-1)
    assert changed.any() and not changed[:, :16].any() and not changed[:, 64:].any()
    ys, xs = np.nonzero(changed)
    assert (np.abs(ys - 16) <= 16).all() and (np.abs(xs - 32) <= 16).all()     # nothing beyond a tile's side from the fast pixel


# ------------------------------------------------------------------ step 4 against the restatement
@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
def test_gather_equals_the_restatement(ftn, size):
    """|got - want| <= (taps + 16) 2^-23 max|colour| over the pixel's centre and taps: per tap one rounding of the running sum, a handful in
    its weight and one in its product, and one final divide"""
    w, h = size
    img = R.image(w, h)
    worst = 0.0
    for name in R.FIELDS:
        m = R.field(name, w, h)
        for gb in (None, R.gbuffer(w, h)):
            for taps in R.TAPS:
                got = V.vector_blur_cpu(ftn, img, m, gb, dict(taps=taps))
                want, copied, peak = R.blur(img, m, gb, taps=taps)
                assert np.array_equal(bits(got)[copied], bits(img)[copied]), (name, taps)
                err = np.abs(got.astype(np.float64) - want).max(-1)
                bound = (taps + 16) * EPS * peak
                worst = max(worst, float((err / bound).max()))
                assert (err <= bound).all(), (name, gb is not None, taps, float((err / bound).max()))
                if taps == 1:
                    assert copied.all()                                       # the only tap is the centre
                elif min(w, h) > 1 and name != "fast_tile":
                    assert not copied.all(), (name, taps)
    print("%dx%d: the largest error is %.3f of the bound" % (w, h, worst))


def test_other_parameters(ftn):
    w, h = 48, 48
    img, gb = R.image(w, h), R.gbuffer(w, h)
    for p in (dict(shutter=1.0), dict(shutter=0.1), dict(max_radius=2.0), dict(max_radius=0.75, shutter=1.0), dict(depth_extent=1.0), dict(depth_extent=1e-6),
              dict(taps=7, shutter=0.9, max_radius=9.5, depth_extent=0.05)):
        for name in ("rotational", "beyond_clamp"):
            m = R.field(name, w, h)
            got = V.vector_blur_cpu(ftn, img, m, gb, p)
            want, copied, peak = R.blur(img, m, gb, **p)
            assert np.array_equal(bits(got)[copied], bits(img)[copied]), p
            assert (np.abs(got.astype(np.float64) - want).max(-1) <= (p.get("taps", 16) + 16) * EPS * peak).all(), p


# ------------------------------------------------------------------ constants
def test_constants(ftn):
    w, h = 80, 48
    for taps in (2, 16, 64):
        for c in (0.75, 3.1, 1000.3):
            img = np.full((h, w, 3), c, F32)
            for name in R.FIELDS:
                got = V.vector_blur_cpu(ftn, img, R.field(name, w, h), R.gbuffer(w, h), dict(taps=taps))
                assert np.abs(got.astype(np.float64) - float(F32(c))).max() <= (taps + 2) * EPS * c, (taps, c, name)
        # constant along x, uniform horizontal motion, one depth: pixels all of whose taps lie inside the image keep their row's value
        rows = R.image(1, h, seed=11)
        img = np.ascontiguousarray(np.broadcast_to(rows, (h, w, 3)))
        m = np.zeros((h, w, 2), F32)
        m[..., 0] = 48.0                                                      # half velocity 12 pixels
        got = V.vector_blur_cpu(ftn, img, m, None, dict(taps=taps))
        inside = slice(12, w - 12)
        err = np.abs(got.astype(np.float64) - img)[:, inside]
        assert (err <= (taps + 2) * EPS * np.abs(img[:, inside])).all(), taps


# ------------------------------------------------------------------ threads
def test_thread_count_changes_no_bit(ftn, monkeypatch):
    w, h = 400, 400                                                           # enough pixels and tiles for several host threads
    img, m, gb = R.image(w, h), R.field("rotational", w, h), R.gbuffer(w, h)
    monkeypatch.setenv("FTN_BVH_THREADS", "1")
    one = V.vector_blur_cpu(ftn, img, m, gb)
    rec = V.velocities_cpu(ftn, m, gb)
    for threads in ("3", "7"):
        monkeypatch.setenv("FTN_BVH_THREADS", threads)
        assert np.array_equal(bits(V.vector_blur_cpu(ftn, img, m, gb)), bits(one)), threads
        again = V.velocities_cpu(ftn, m, gb)
        assert all(np.array_equal(bits(again[k]), bits(rec[k])) for k in rec), threads
    monkeypatch.delenv("FTN_BVH_THREADS")
    assert np.array_equal(bits(V.vector_blur_cpu(ftn, img, m, gb)), bits(one))
    assert not np.array_equal(bits(one), bits(img))
