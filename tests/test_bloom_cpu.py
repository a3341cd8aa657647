"""The host twin of the bloom stage (ftn_bloom_cpu, which shares its per-pixel code with the kernels) without a GPU: against the binary64
restatement tests/_bloom_ref.py over sizes, levels, flags, thresholds and scatters, within bounds measured on the twin; the exact
properties (copies, constants, scatter 0, symmetry, thread count); the conservation of energy and its loss under the Karis flag; the
salted image; the threshold's knee; the Karis flag's firefly suppression."""
import itertools

import numpy as np
import pytest

from fountain_amd import bloom as B

import _bloom_common as K
import _bloom_ref as R

F32 = np.float32
EPS32 = float(np.finfo(F32).eps)
bits = K.bits


# ------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: "%dx%d" % s)
def test_twin_against_the_restatement(ftn, size):
    w, h = size
    img = K.image(w, h)
    before = img.copy()
    worst = {False: 0.0, True: 0.0}
    for lv, karis, th, sc in itertools.product(K.LEVELS, (False, True), K.THRESHOLDS, K.SCATTERS):
        kw = dict(levels=lv, scatter=sc, strength=0.5, **th)
        got = B.bloom_cpu(ftn, img, dict(karis=karis, **kw))
        e = K.err(got, R.bloom(img, R.params(karis=karis, **kw)))
        worst[karis] = max(worst[karis], e)
        assert np.isfinite(got).all() and e <= (K.BOUND_KARIS if karis else K.BOUND_PLAIN), (size, lv, karis, th, sc, e)
    print("bloom twin against the restatement, %dx%d: %.3g plain, %.3g karis" % (w, h, worst[False], worst[True]))
    assert np.array_equal(bits(img), bits(before))


def test_measurements_are_current(ftn):
    """the two cases of the sweep above that gave the largest errors, again: they must still give MEASURED_PLAIN and MEASURED_KARIS (to
    the three digits kept), so that the bounds, four times those, cannot drift from what the twin does"""
    img = K.image(255, 257)
    for karis, measured, kw in ((False, K.MEASURED_PLAIN, dict(levels=6, scatter=1.0, threshold=1.0, knee=0.5)),
                                (True, K.MEASURED_KARIS, dict(levels=1, scatter=0.0, threshold=1.0, knee=0.0))):
        e = K.err(B.bloom_cpu(ftn, img, dict(karis=karis, strength=0.5, **kw)), R.bloom(img, R.params(karis=karis, strength=0.5, **kw)))
        print("bloom twin, the worst case %s the Karis flag: %.4g (recorded %.3g)" % ("with" if karis else "without", e, measured))
        assert 0.99 * measured <= e <= measured, (karis, e, measured)
    assert K.BOUND_PLAIN == 4 * K.MEASURED_PLAIN and K.BOUND_KARIS == 4 * K.MEASURED_KARIS


# ------------------------------------------------------------------ exact properties
def test_exact_copies(ftn):
    img = K.image(17, 31)
    img[3, 4] = (-0.0, 0.0, -0.0)
    img[5, 6] = np.array([0x7fc12345, 0xffc00001, 0x7f800001], np.uint32).view(F32)          # NaNs with payloads
    img[7, 8] = (np.inf, -np.inf, -3.0)
    for p in (dict(strength=0.0), dict(levels=0), dict(strength=0.0, karis=True, threshold=1.0), dict(levels=0, strength=1.0)):
        assert np.array_equal(bits(B.bloom_cpu(ftn, img, p)), bits(img)), p
    one = np.array([0x80000000, 0x7fc12345, 0x3f800000], np.uint32).view(F32).reshape(1, 1, 3)
    for p in (dict(), dict(strength=1.0, levels=12, karis=True)):
        assert np.array_equal(bits(B.bloom_cpu(ftn, one, p)), bits(one)), p


@pytest.mark.parametrize("c", [0.0, 0.75, 1.0, 3.0, 1024.0])
def test_constants_come_back(ftn, c):
    """all weights are dyadic and sum to 1, so every level of a constant image is the constant and B - P is 0 (with a scatter that is
    not dyadic a level may be off by an ulp, which strength 0.04 takes below half an ulp of c)"""
    img = np.full((53, 37, 3), c, F32)
    for lv, sc in itertools.product(range(0, 13), K.SCATTERS):
        assert np.array_equal(bits(B.bloom_cpu(ftn, img, dict(levels=lv, scatter=sc))), bits(img)), (c, lv, sc)
    for lv, sc in itertools.product((1, 2, 6, 12), (0.0, 0.5, 1.0)):                        # dyadic scatters: exact at full strength too
        assert np.array_equal(bits(B.bloom_cpu(ftn, img, dict(levels=lv, scatter=sc, strength=1.0))), bits(img)), (c, lv, sc)


def test_scatter_zero_is_the_first_level_alone(ftn):
    """U_1 = D_1 * 1 + up(U_2) * 0 = D_1, so the deeper levels change no bit, and B = up(D_1)"""
    img = K.image(64, 64)
    one = B.bloom_cpu(ftn, img, dict(levels=1, scatter=0.0, strength=1.0))
    for lv in (2, 6, 12):
        assert np.array_equal(bits(B.bloom_cpu(ftn, img, dict(levels=lv, scatter=0.0, strength=1.0))), bits(one)), lv
    assert np.array_equal(bits(B.bloom_cpu(ftn, img, dict(levels=1, scatter=0.7, strength=1.0))), bits(one))   # level 1 is the last: nothing to blend
    p = R.params(levels=1, strength=1.0)
    want = img.astype(np.float64) + (R.up(R.down(R.prefilter(img, p)), 64, 64) - R.prefilter(img, p))
    assert K.err(one, want) <= K.BOUND_PLAIN
    assert not np.array_equal(bits(B.bloom_cpu(ftn, img, dict(levels=2, scatter=0.7, strength=1.0))), bits(one))


def test_symmetry_of_a_centred_block(ftn):
    """a centred 2 x 2 block on 64 x 64: the bloom is symmetric under both flips and the transpose.  The header fixes the order of every
    sum (rows outer, columns inner, ascending) and a flip reverses it, so the symmetry is bit for bit exactly where every sum is exact:
    the block a power of two, scatter and strength dyadic like the weights, no Karis quotient.  With the default scatter 0.7 or the
    Karis flag the mirrored sums round differently, and the symmetry holds within the twin's bound instead"""
    img = np.zeros((64, 64, 3), F32)
    img[31:33, 31:33] = (1024.0, 512.0, 2048.0)
    flips = lambda out: (("left-right", out[:, ::-1]), ("up-down", out[::-1]), ("transpose", out.transpose(1, 0, 2)))
    for p in (dict(levels=1, strength=1.0), dict(levels=2, scatter=0.5, strength=0.5), dict(levels=3, scatter=0.75, strength=0.25),
              dict(levels=6, scatter=0.5, strength=0.5), dict(levels=12, scatter=1.0, strength=1.0)):
        out = B.bloom_cpu(ftn, img, p)
        assert (out[31:33, 31:33] != img[31:33, 31:33]).all() and out[31, 30, 0] > 0
        for name, other in flips(out):
            assert np.array_equal(bits(other), bits(out)), (p, name)
    for p in (dict(strength=0.5), dict(strength=0.5, karis=True), dict(strength=0.5, threshold=1.0)):
        out = B.bloom_cpu(ftn, img, p)
        for name, other in flips(out):
            assert K.err(other, out) <= (K.BOUND_KARIS if p.get("karis") else K.BOUND_PLAIN), (p, name)
    sym = R.bloom(img, R.params(strength=0.5))
    assert max(K.err(other, sym) for _, other in flips(sym)) <= 1e-12


def test_thread_count_changes_no_bit(ftn, monkeypatch):
    img = K.image(400, 400)                                                        # enough pixels for several host threads
    p = dict(karis=True, threshold=1.0, strength=0.5)
    monkeypatch.setenv("FTN_BVH_THREADS", "1")
    one = B.bloom_cpu(ftn, img, p)
    for threads in ("3", "7"):
        monkeypatch.setenv("FTN_BVH_THREADS", threads)
        assert np.array_equal(bits(B.bloom_cpu(ftn, img, p)), bits(one)), threads
    monkeypatch.delenv("FTN_BVH_THREADS")
    assert np.array_equal(bits(B.bloom_cpu(ftn, img, p)), bits(one))


# ------------------------------------------------------------------ energy
def impulses(L, size=128):
    """impulses at least 2^(L + 1) pixels from every border"""
    m = 2 ** (L + 1)
    img = np.zeros((size, size, 3), F32)
    for (x, y), v in (((m, m), (1000.0, 1000.0, 1000.0)), ((size - 1 - m, m + 5), (37.5, 2000.0, 3.0)), ((size // 2 + 1, size - 1 - m), (1e4, 1e4, 1e4)),
                      ((size // 2, size // 2), (5.0, 700.0, 90.0))):
        img[y, x] = v
    return img


@pytest.mark.parametrize("th", [dict(threshold=0.0), dict(threshold=2.0, knee=0.5)], ids=["no threshold", "threshold"])
@pytest.mark.parametrize("L", [1, 3, 4])
def test_energy_is_conserved_away_from_the_borders(ftn, L, th):
    img = impulses(L)
    total = float(img.astype(np.float64).sum())
    for sc, st in ((0.7, 0.04), (1.0, 1.0), (0.3, 0.5)):
        kw = dict(levels=L, scatter=sc, strength=st, **th)
        ref = R.bloom(img, R.params(**kw))
        assert abs(ref.sum() - total) <= 1e-12 * total, (L, kw)
        got = B.bloom_cpu(ftn, img, kw).astype(np.float64)
        print("bloom energy, L %d %s: twin %.3g eps, restatement %.3g" % (L, kw, abs(got.sum() - total) / (EPS32 * total), abs(ref.sum() - total) / total))
        assert abs(got.sum() - total) <= 16 * EPS32 * total, (L, kw, abs(got.sum() - total) / (EPS32 * total))
        assert (got != img).sum() > 3 * 16


def test_karis_gives_energy_up(ftn):
    """the luminance-weighted first step is normalised per output, not per source: next to a 10^4 impulse energy is lost"""
    img = np.full((128, 128, 3), 0.1, F32)
    img[64, 63] = 1e4
    total = float(img.astype(np.float64).sum())
    kw = dict(levels=4, strength=1.0)
    for run in (lambda k: R.bloom(img, R.params(karis=k, **kw)), lambda k: B.bloom_cpu(ftn, img, dict(karis=k, **kw)).astype(np.float64)):
        assert total - run(True).sum() > 0.1 * total
        # without the flag only what the clamped borders lose or gain of the 0.1 field is missing, which is exact for a constant: nothing
        assert abs(run(False).sum() - total) <= 16 * EPS32 * total


# ------------------------------------------------------------------ the salted image
@pytest.mark.parametrize("p", [dict(strength=0.5), dict(strength=0.5, karis=True, threshold=1.0, levels=3)], ids=["plain", "karis threshold"])
def test_salted_image(ftn, p):
    img, clean = K.salted()
    out = B.bloom_cpu(ftn, img, p)
    with np.errstate(invalid="ignore"):
        stays = ~np.isfinite(img) | (img < 0)
    assert stays.sum() >= 16 and (~stays).sum() > 5000
    assert np.array_equal(bits(out)[stays], bits(img)[stays])                       # NaN, +-inf and negatives: the same bits
    assert np.isfinite(out[~stays]).all()
    # nothing leaks: every other channel is what it is on the image whose salted channels hold what the prefilter makes of them
    assert np.array_equal(bits(out)[~stays], bits(B.bloom_cpu(ftn, clean, p))[~stays])
    assert K.err(out[~stays], R.bloom(img, R.params(**p))[~stays]) <= (K.BOUND_KARIS if p.get("karis") else K.BOUND_PLAIN)
    # the successor of clamp_max is clamped: the same bloom around it as around clamp_max itself
    a = np.zeros((9, 9, 3), F32)
    b = a.copy()
    a[4, 4], b[4, 4] = 65504.0, np.nextafter(F32(65504.0), F32(np.inf))
    oa, ob = B.bloom_cpu(ftn, a, dict(strength=1.0, levels=2)), B.bloom_cpu(ftn, b, dict(strength=1.0, levels=2))
    mask = np.ones((9, 9), bool)
    mask[4, 4] = False
    assert np.array_equal(bits(oa)[mask], bits(ob)[mask]) and oa[3, 4, 0] > 0


# ------------------------------------------------------------------ the threshold
def neighbour_response(ftn, v, **kw):
    """what a grey pixel of value v in a black 8 x 8 image sends to the pixel beside it: a fixed positive multiple of P(v)"""
    img = np.zeros((8, 8, 3), F32)
    img[4, 4] = v
    return float(B.bloom_cpu(ftn, img, dict(levels=1, strength=1.0, **kw))[4, 5, 1])


@pytest.mark.parametrize("knee", [0.25, 0.5, 1.0])
def test_knee_is_continuous(ftn, knee):
    t, Kk = 1.0, knee * 1.0
    scale = neighbour_response(ftn, F32(t + Kk), threshold=t, knee=knee)
    assert scale > 0
    for centre in (t + Kk, t - Kk):
        vs = [F32(centre)]
        for _ in range(16):
            vs = [np.nextafter(vs[0], F32(-np.inf))] + vs + [np.nextafter(vs[-1], F32(np.inf))]
        lum = [F32(F32(v * F32(0.212671)) + F32(v * F32(0.715160))) + F32(v * F32(0.072169)) for v in vs]
        assert lum[0] < F32(centre) < lum[-1]                                     # the sweep crosses the branch
        f = [neighbour_response(ftn, v, threshold=t, knee=knee) for v in vs]
        assert all(b >= a for a, b in zip(f, f[1:])) or centre == 0.0
        assert max(abs(b - a) for a, b in zip(f, f[1:])) <= 16 * EPS32 * scale, (knee, centre)
    # far above the knee the response is that of Y - threshold
    assert neighbour_response(ftn, F32(101.0), threshold=t, knee=knee) == pytest.approx(100.0 / 101.0 * neighbour_response(ftn, F32(101.0)), rel=1e-5)


def test_below_the_knee_nothing_blooms(ftn):
    rng = np.random.default_rng(5)
    img = rng.uniform(0.0, 0.5, (31, 17, 3)).astype(F32)                           # Y <= 0.5 = threshold - K
    img[3, 3] = 0.5
    p = dict(threshold=1.0, knee=0.5, strength=1.0)
    assert np.array_equal(bits(B.bloom_cpu(ftn, img, p)), bits(img))
    assert np.array_equal(bits(B.bloom_cpu(ftn, img, dict(threshold=1.0, knee=0.0, strength=1.0, karis=True))), bits(img))
    img[10, 10] = 0.75                                                             # inside the knee: it blooms, and only it
    out = B.bloom_cpu(ftn, img, p)
    assert out[10, 10, 0] < img[10, 10, 0] and out[10, 11, 0] > img[10, 11, 0]
    lone = np.zeros_like(img)
    lone[10, 10] = 0.75
    # what it adds to the others is what it adds to a black image, up to the rounding of in + B at values below 1
    assert np.abs((out.astype(np.float64) - img) - (B.bloom_cpu(ftn, lone, p).astype(np.float64) - lone)).max() <= EPS32


# ------------------------------------------------------------------ Karis
def test_karis_suppresses_a_firefly(ftn):
    img = np.full((64, 64, 3), 0.1, F32)
    img[32, 31] = 1e4
    factor = {}
    for karis in (False, True):
        kw = dict(levels=6, strength=0.04)
        ref = R.bloom(img, R.params(karis=karis, **kw))
        got = B.bloom_cpu(ftn, img, dict(karis=karis, **kw))
        assert K.err(got, ref) <= (K.BOUND_KARIS if karis else K.BOUND_PLAIN)
        factor[karis] = (float(ref[32, 33, 0]) / 0.1, float(got[32, 33, 0]) / 0.1)
    print("bloom firefly: neighbour raised %.4g x without the flag, %.4g x with it" % (factor[False][0], factor[True][0]))
    for k, karis in itertools.product((0, 1), (False, True)):                     # the restatement, then the twin
        assert 1.0 <= factor[True][k] < factor[False][k]
        assert abs(factor[karis][1] - factor[karis][0]) <= K.BOUND_KARIS * factor[karis][0]
