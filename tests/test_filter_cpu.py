"""The host twin of the reconstruction-filtered film (ftn_filter_accumulate_samples, include/fountain_hip_filter.h) without a GPU, fed
with the CPU oracle's radiance of every camera sample (orc_render_sample_log): bit for bit against a float32 numpy restatement that shares
no code with the library (_filter_ref.py); against float64 within the derived bound; the box of radius 0.5 against the beauty's own
sums; a constant scene under every filter; invariance under the order of the input and the number of threads; and the variance of a
filtered pixel on synthetic samples against sigma^2 sum w^2 / (sum w)^2."""
import numpy as np
import pytest

from fountain_amd import DirectLightingIntegrator, PathIntegrator, PerspectiveCamera, RandomSampler, WhittedIntegrator, scenes
from fountain_amd import filters as FL

import _filter_ref as FR
import _gbuffer_ref as GR
import _moments_ref as MR
from test_moments_cpu import constant_sphere

F32 = np.float32
bits = MR.bits
FULL = (0.0, 0.0, 1.0, 1.0)
CROP = (0.1, 0.05, 0.9, 0.95)          # cuts tiles on every side
INTEGRATORS = {"path": lambda: PathIntegrator(5, 1.0), "direct": lambda: DirectLightingIntegrator(4), "whitted": lambda: WhittedIntegrator(4)}


def make_scene(which):
    """cornell at 40 x 40, and the odd 17 x 33, row 37 x 1 and col 1 x 37 films of test_moments_oracle.py"""
    res = {"cornell": (40, 40), "odd": (17, 33), "row": (37, 1), "col": (1, 37)}[which]

    def make(be):
        b, cam, _ = scenes.cornell(be, res=40)
        if which != "cornell":
            cam = PerspectiveCamera.look_at(be, (0.0, -3.4, 0.0), (0.0, 0.0, 0.0), (0, 0, 1), res, fov=40.0)
        return b, cam, res
    return make


# scene, integrator, filter kind, radius, crop, tiles, spp, first, count
CASES = [
    ("cornell", "path", "box", (0.5, 0.5), FULL, None, 4, 0, 0),
    ("cornell", "path", "gaussian", (2.0, 2.0), FULL, None, 4, 0, 0),
    ("cornell", "direct", "mitchell", (2.0, 2.0), CROP, None, 6, 1, 4),
    ("cornell", "whitted", "sinc", (4.0, 4.0), CROP, (1, 2, 0), 3, 0, 0),
    ("cornell", "path", "triangle", (1.5, 1.5), FULL, (1, 2, 0), 4, 0, 0),
    ("cornell", "direct", "gaussian", (1.5, 0.75), (0.0, 0.1, 0.85, 1.0), None, 4, 0, 0),
    ("cornell", "path", "sinc", (8.0, 8.0), CROP, None, 2, 0, 0),
    ("cornell", "path", "mitchell", (8.0, 8.0), FULL, (1, 2, 0), 2, 0, 0),
    ("odd", "path", "mitchell", (1.5, 0.75), FULL, (1, 2, 0), 5, 2, 3),
    ("odd", "whitted", "box", (2.0, 2.0), FULL, None, 3, 0, 0),
    ("odd", "path", "triangle", (4.0, 4.0), CROP, None, 3, 0, 0),
    ("row", "path", "gaussian", (2.0, 2.0), FULL, None, 4, 0, 0),
    ("row", "direct", "sinc", (4.0, 4.0), FULL, None, 3, 0, 0),
    ("row", "path", "box", (0.5, 0.5), FULL, None, 4, 0, 0),
    ("col", "path", "mitchell", (1.5, 1.5), FULL, None, 4, 0, 0),
    ("col", "whitted", "triangle", (8.0, 8.0), FULL, None, 2, 0, 0),
    ("col", "direct", "gaussian", (1.5, 0.75), FULL, (1, 2, 0), 4, 0, 0),
    ("cornell", "path", "gaussian", (1.75, 1.75), FULL, None, 3, 0, 0),      # floor(r + 0.5) = 2 where floor(r) = 1: the margin formula itself
]
_records = {}


def records(orc_det, which, integ, radius, crop, tiles, spp, first, count, seed=17):
    """the oracle's sample log of a case, computed once and shared by the tests (read-only)"""
    key = (which, integ, radius, crop, tiles, spp, first, count, seed)
    if key not in _records:
        smp = RandomSampler(spp, seed, indexed=True, first_sample=first, sample_count=count)
        rec, film, _ = MR.oracle_records(orc_det, make_scene(which), INTEGRATORS[integ](), smp, crop, radius, tiles)
        rec.setflags(write=False)
        _records[key] = (rec, film)
    return _records[key]


def twin(ftn, film, filt, rec, out=None):
    return FL.accumulate_samples(ftn, film, filt, rec["px"], rec["py"], rec["sample"], rec["p_film"], rec["L"], out)


def case_filter(ftn, kind, radius):
    return FL.Filter(kind, radius, be=ftn)


@pytest.mark.parametrize("which,integ,kind,radius,crop,tiles,spp,first,count", CASES)
def test_twin_against_numpy(ftn, orc_det, which, integ, kind, radius, crop, tiles, spp, first, count):
    """(a) bit for bit against the float32 restatement, filter_weight_sum included; (b) against float64 within gamma(n + 3) sum |w L|"""
    rec, film = records(orc_det, which, integ, radius, crop, tiles, spp, first, count)
    filt = case_filter(ftn, kind, radius)
    got = twin(ftn, film, filt, rec)
    ref = FR.film_ref(film, filt.table(), rec)                         # the library's own table (within 1 ulp of float64: test_filter_abi.py)
    diff = (bits(got) != bits(ref["pixels"])).any(-1)
    assert not diff.any(), "%d pixels differ, first %r: %r vs %r" % (int(diff.sum()), tuple(np.argwhere(diff)[0]), got[tuple(np.argwhere(diff)[0])],
                                                                       ref["pixels"][tuple(np.argwhere(diff)[0])])
    FR.assert_within(got, ref, what="%s/%s" % (which, kind))
    assert ref["terms"].max() > spp or radius[0] == 0.5                # a wide filter gathers from neighbours
    assert (ref["terms"] > 0).any()
    if tiles is not None and max(radius) < 8:                          # (at radius 8 every pixel of a skipped 16-pixel tile is reached)
        assert (ref["terms"] == 0).any()                               # pixels out of every selected tile's reach stay empty ...
        assert not got[ref["terms"] == 0].any()
    if kind in ("mitchell", "sinc"):
        assert (ref["magw"] > np.abs(ref["w64"]) * (1 + 1e-6)).any()   # ... and negative weights did take part


def test_box_equals_the_beauty(ftn, orc_det):
    """(c) a box of radius 0.5 through the twin equals the beauty's sums (_moments_ref.gpu_sums) bit for bit wherever no sample of
    another pixel landed"""
    for which, integ, crop, tiles in (("cornell", "path", FULL, None), ("cornell", "direct", CROP, (1, 2, 0)), ("odd", "whitted", FULL, None),
                                     ("row", "path", FULL, None)):
        rec, film = records(orc_det, which, integ, (0.5, 0.5), crop, tiles, 4, 0, 0)
        got = twin(ftn, film, case_filter(ftn, "box", None), rec)
        ref = MR.gpu_sums(film, GR.selected_tiles(film, tiles), rec)
        own = ~ref["foreign"]
        assert own.sum() >= own.size - 8 and np.array_equal(bits(got[own]), bits(ref["beauty"][own])), which
        assert np.array_equal(bits(got[..., 3]), bits(ref["beauty"][..., 3]))


def resolve_bound(ref, L):
    """|ftn_film_resolve(film) - L| per pixel and rgb channel for a scene of constant radiance L, first order, from the bound of (b):
    the film's xyz lie within B of M S (S = L sum w the exact rgb sums, M = RGB2XYZ) and its weight within Bw of sum w; xyz_to_rgb adds
    three roundings through |XYZ2RGB| and inverts M only to E = |XYZ2RGB M - 1|; 1 / W and the product round once each."""
    B = FR.sum_bound(ref)
    Mi, Mf = MR.XYZ2RGB.astype(np.float64), MR.RGB2XYZ.astype(np.float64)
    E = np.abs(Mi @ Mf - np.eye(3))
    L = np.asarray(L, np.float64)
    W = np.abs(ref["w64"])[..., None]
    S = np.abs(ref["w64"])[..., None] * L
    with np.errstate(all="ignore"):
        e_rgb = B[..., :3] @ np.abs(Mi).T + MR.gamma(3) * ((np.abs(ref["xyz64"]) + B[..., :3]) @ np.abs(Mi).T) + S @ E.T
        return (e_rgb / W + L * B[..., 3:] / W + 3 * MR.U * L) * (1 + 1e-3)


@pytest.mark.parametrize("kind", FR.KINDS)
def test_constant_radiance_resolves_to_the_constant(ftn, orc_det, kind):
    """(d) every camera sample returns L, so every pixel's weighted mean is L whatever the weights, Mitchell's and the sinc's negative
    lobes included"""
    L = (0.7, 1.3, 2.1)
    key = ("const", kind)
    filt = case_filter(ftn, kind, None)
    if key not in _records:
        _records[key] = MR.oracle_records(orc_det, lambda be: constant_sphere(be, res=24, L=L), PathIntegrator(3, 1.0), RandomSampler(4, 5, indexed=True),
                                          FULL, filt.radius)[:2]
    rec, film = _records[key]
    assert np.array_equal(rec["L"], np.broadcast_to(np.array(L, F32), rec["L"].shape))
    film.pixels[...] = 0
    twin(ftn, film, filt, rec, film.pixels)
    ref = FR.film_ref(film, filt.table(), rec)
    rgb = film.into_spectrum_buffer()[0].astype(np.float64)
    err = np.abs(rgb - np.array(L))
    bound = resolve_bound(ref, L)
    assert (ref["w64"] > 0).all() and (err <= bound).all(), float((err / bound).max())
    assert bound.max() < 1e-3                                          # (the sinc: 256 terms a pixel, sum |w| well above sum w)


def test_input_order_and_threads_change_no_bit(ftn, orc_det, monkeypatch):
    """(e) the twin orders its input itself; (f) each output pixel is summed by one thread from its own terms"""
    rec, film = records(orc_det, "cornell", "direct", (2.0, 2.0), CROP, None, 6, 1, 4)
    filt = case_filter(ftn, "mitchell", (2.0, 2.0))
    monkeypatch.setenv("FTN_BVH_THREADS", "1")
    base = twin(ftn, film, filt, rec)
    rng = np.random.default_rng(3)
    for threads in ("1", "2", "7", "32"):
        monkeypatch.setenv("FTN_BVH_THREADS", threads)
        for perm in (np.arange(len(rec)), np.arange(len(rec))[::-1], rng.permutation(len(rec))):
            assert np.array_equal(bits(twin(ftn, film, filt, rec[perm])), bits(base)), threads
    # adding into a buffer: the call's film from zero, added once
    monkeypatch.delenv("FTN_BVH_THREADS")
    start = rng.uniform(-1, 1, base.shape).astype(F32)
    assert np.array_equal(bits(twin(ftn, film, filt, rec, start.copy())), bits((start + base).astype(F32)))


@pytest.mark.parametrize("kind,radius", [("gaussian", (2.0, 2.0)), ("mitchell", (2.0, 2.0)), ("box", (0.5, 0.5)), ("triangle", (1.5, 0.75))])
def test_variance_of_a_filtered_pixel(ftn, kind, radius):
    """(g) synthetic records: one sample per source pixel and sample index at a uniformly jittered position, radiance mu + sigma N(0, 1),
    independent.  Given the positions a pixel's resolved value is mu + sum w e / sum w, so d^2 = (value - mu)^2 has expectation
    sigma^2 sum w^2 / (sum w)^2 computed from the weights that actually covered the pixel.  Over K independent pixels (interior pixels
    further apart than two footprints, several seeds) the mean of z = d^2 - sigma^2 sum w^2 / (sum w)^2 is 0: it must lie within five
    standard errors of z's mean, estimated from the K values."""
    filt = case_filter(ftn, kind, radius)
    res, spp, mu, sigma = 64, 4, 1.0, 0.5
    film = FL.filtered_film(ftn, filt, (res, res))
    sb = film.sample_bounds()
    ys, xs = np.mgrid[sb[1]:sb[3], sb[0]:sb[2]]
    step = 2 * int(np.ceil(max(radius))) + 2
    pick = np.arange(10, res - 10, step)
    z, pred_all = [], []
    for seed in range(6):
        rng = np.random.default_rng(100 + seed)
        n = xs.size * spp
        rec = np.zeros(n, MR.RECORD)
        rec["px"], rec["py"] = np.tile(xs.ravel(), spp), np.tile(ys.ravel(), spp)
        rec["sample"] = np.repeat(np.arange(spp), xs.size)
        rec["p_film"] = np.stack([rec["px"], rec["py"]], -1).astype(F32) + rng.uniform(0, 1, (n, 2)).astype(F32)
        rec["L"] = (mu + sigma * rng.standard_normal(n)).astype(F32)[:, None]
        got = twin(ftn, film, filt, rec).astype(np.float64)
        ref = FR.film_ref(film, filt.table(), rec)
        value = (got[..., :3] @ MR.XYZ2RGB.astype(np.float64)[1]) / got[..., 3]               # g of xyz_to_rgb(xyz) / W
        d2 = (value - mu) ** 2
        pred = sigma ** 2 * ref["w2"] / ref["w1"] ** 2
        z.append((d2 - pred)[np.ix_(pick, pick)].ravel())
        pred_all.append(pred[np.ix_(pick, pick)].ravel())
    z, pred_all = np.concatenate(z), np.concatenate(pred_all)
    K = len(z)
    se = z.std(ddof=1) / np.sqrt(K)
    assert K >= 200 and abs(z.mean()) <= 5 * se, (z.mean(), se, pred_all.mean())
    # and the filter matters: a wide filter averages more samples than the pixel's own
    if kind != "box":
        assert pred_all.mean() < 0.8 * sigma ** 2 / spp
