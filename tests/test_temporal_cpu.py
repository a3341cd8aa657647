"""The host twin of temporal accumulation (ftn_temporal_accumulate_cpu, include/fountain_hip_temporal.h) against the float64 restatement of
tests/_temporal_ref.py on synthetic frames of analytic cameras, and the properties the header states: the first frame is a copy, equal
cameras give a motion of exactly zero and the recurrence of step 4 bit for bit, no history crosses a depth edge, reprojection stays
within the bilinear interpolation error, the edge inputs, and no dependence on the host thread count.  CPU only."""
import os

import numpy as np
import pytest

from fountain_amd import _abi as A
from fountain_amd import temporal as T

import _temporal_ref as R

SIZES = [(1, 1), (3, 5), (9, 17), (48, 64), (120, 200)]          # (h, w)
TWO_PLANES = [dict(z=2.0, xmax=0.1), dict(z=5.0, xmax=3.0)]      # a near plane over the left half, a far one behind it, sky beyond x = 3
# Twin against restatement, |got - want| / max(|want|, 1e-3) over the pixels that are not fragile: 4 x the largest value measured over
# every case of test_twin_against_restatement on the host (the factor of DESIGN.md section 3.1), not taken from the device.
TWIN_MEASURED_MAX = 1.21e-4
TWIN_BOUND = 4 * TWIN_MEASURED_MAX
FRAGILE_MAX = 0.005


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def cameras(h, w, motion, n=3):
    """n cameras on a short path in front of TWO_PLANES: frame k is moved by k steps; a step shifts the near plane by about `motion`
    pixels along x and 0.8 of that along y, and turns the view by about 0.6 `motion` pixels (no motion
    with a fractional part near zero: a pixel whose heavy taps are refused is left with a weight that is small, not tiny)"""
    f = 0.75 * max(h, w)
    return [R.pinhole((k * motion * 3.0 / f, -0.8 * k * motion * 3.0 / f, -1.0 + 0.02 * k), (w, h), f, yaw=0.6 * k * motion / f, pitch=-0.3 * k * motion / f)
            for k in range(n)]


def sequence(h, w, motion, n=3, seed=0, **kw):
    cams = cameras(h, w, motion, n)
    kw.setdefault("normal_noise", 0.1)
    return cams, [R.make_frame(c, TWO_PLANES, h, w, seed=seed + 31 * k, **kw) for k, c in enumerate(cams)]


def run_twin(ftn, cams, frames, params, origin=(0, 0), check=None):
    """the twin over a sequence; returns the per-frame (history, rgb, var4); check(k, frame, cam, prev, got) sees every frame"""
    h, w = frames[0][0].shape[:2]
    film = R.film_desc(A, (w, h), origin, full=(w + origin[0] + 3, h + origin[1] + 2))
    out, prev, prev_ref = [], None, None
    for k, (cam, fr) in enumerate(zip(cams, frames)):
        got = T.temporal_accumulate_cpu(ftn, *fr, R.camera_desc(A, cam), film, prev, params)
        if check:
            check(k, fr, cam, prev_ref, got)
        prev, prev_ref = (R.camera_desc(A, cam), fr[1], got[0]), (cam, fr[1], got[0])
        out.append(got)
    return out


# ------------------------------------------------------------------ 1. twin against the restatement
def test_twin_against_restatement(ftn):
    """every size, both flags, three alpha_min, sub-pixel and multi-pixel motion, a crop origin: each frame of the twin against the
    restatement fed with the twin's own history, so that errors do not compound"""
    tally = dict(pixels=0, fragile=0, worst=0.0)
    for h, w in SIZES:
        compared = 0
        for motion in (0.3, 4.7):
            cams, frames = sequence(h, w, motion, seed=1000 * h + w)
            for flags in (0, 1):
                for alpha_min in (0.0, 0.2, 1.0):
                    p = dict(flags=flags, alpha_min=alpha_min, normal_tol=0.05, plane_tol=0.004, albedo_tol=0.003 if alpha_min else 0.05)
                    origin = (0, 0) if flags else (7, 3)

                    def check(k, fr, cam, prev, got):
                        nonlocal compared
                        want = R.reference(*fr, cam, origin, prev, **p)
                        ok = ~want[3]
                        tally["pixels"] += ok.size
                        tally["fragile"] += int((~ok).sum())
                        compared += int(ok.sum())
                        for g, x in zip(got, want[:3]):
                            tally["worst"] = max(tally["worst"], R.rel_error(g[ok], x[ok]))
                    run_twin(ftn, cams, frames, p, origin, check)
        assert compared > 0, (h, w)
    print("twin against restatement: worst relative error %.3g, %d of %d pixels left out as fragile (%.4f %%)"
          % (tally["worst"], tally["fragile"], tally["pixels"], 100.0 * tally["fragile"] / tally["pixels"]))
    assert tally["fragile"] <= FRAGILE_MAX * tally["pixels"]
    assert tally["worst"] <= TWIN_BOUND


def test_restatement_alone_leaves_out_little():
    """the synthetic cameras keep the restatement's own count of fragile pixels under 0.5 %, at the sizes where a single pixel is less
    than that, for histories the restatement made itself"""
    for h, w in SIZES[3:]:
        for motion in (0.3, 4.7):
            cams, frames = sequence(h, w, motion, seed=5)
            prev, n = None, 0
            for cam, fr in zip(cams, frames):
                hist, _, _, fragile = R.reference(*fr, cam, (0, 0), prev, normal_tol=0.05, plane_tol=0.004)
                n += int(fragile.sum())
                prev = (cam, fr[1], hist.astype(np.float32))
            assert n <= FRAGILE_MAX * 3 * h * w, (h, w, motion, n)


def test_history_is_found_and_rejected(ftn):
    """the sequences of test 1 exercise what they are meant to: most pixels find history, some are refused it by each rule"""
    cams, frames = sequence(120, 200, 4.7, seed=9)
    strict = run_twin(ftn, cams, frames, dict(alpha_min=0.0, normal_tol=0.05, plane_tol=0.004, albedo_tol=1.0))
    loose = run_twin(ftn, cams, frames, dict(alpha_min=0.0, normal_tol=4.0, plane_tol=0.004, albedo_tol=1.0))
    flat = run_twin(ftn, cams, frames, dict(alpha_min=0.0, normal_tol=4.0, plane_tol=100.0, albedo_tol=1.0))
    same = run_twin(ftn, cams, frames, dict(alpha_min=0.0, normal_tol=0.05, plane_tol=0.004, albedo_tol=0.002))
    free = run_twin(ftn, cams, frames, dict(flags=0, alpha_min=0.0, normal_tol=0.05, plane_tol=0.004, albedo_tol=0.0))
    n = [x[2][0][..., 3] for x in (strict, loose, flat)]
    # the divisor test converts some taps, refuses none, and acts only when demodulating
    assert np.array_equal(same[2][0][..., 3], n[0]) and not np.array_equal(bits(same[2][1]), bits(strict[2][1]))
    assert np.array_equal(free[2][0][..., 3], n[0])
    off = run_twin(ftn, cams, frames, dict(flags=0, alpha_min=0.0, normal_tol=0.05, plane_tol=0.004, albedo_tol=1.0))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(free[2], off[2]))
    assert (n[0] > 2).mean() > 0.5 and (n[0] == 1).any()
    assert (n[1] > n[0]).any() and (n[2] > n[1]).any()                   # the normal test and the plane test each refuse some taps
    cov = frames[2][1][..., 10] > 0
    assert (~cov).any() and (n[0][~cov] > 1).any()                       # uncovered pixels accumulate too


# ------------------------------------------------------------------ 2. the first frame
@pytest.mark.parametrize("h,w", SIZES)
def test_first_frame_is_a_copy(ftn, h, w):
    cams, frames = sequence(h, w, 1.0, n=1, seed=h + w)
    rgb, gb, var = frames[0]
    hist, out, ovar = run_twin(ftn, cams, frames, dict(flags=0))[0]
    assert np.array_equal(bits(out), bits(rgb)) and np.array_equal(bits(ovar), bits(var))
    assert (hist[..., 3] == 1).all()
    assert np.array_equal(bits(hist[..., :3]), bits(rgb)) and np.array_equal(bits(hist[..., 4:]), bits(var))
    hist, out, ovar = run_twin(ftn, cams, frames, dict(flags=1))[0]
    assert (hist[..., 3] == 1).all() and np.array_equal(bits(ovar[..., 3]), bits(var[..., 3]))
    assert R.rel_error(out, rgb) <= 2.0 ** -22 and R.rel_error(ovar, var) <= 2.0 ** -21       # a quotient and a product back: 2 and 4 roundings


# ------------------------------------------------------------------ 3. equal cameras
def recurrence(frames, flags, alpha_min, eps=np.float32(1e-3)):
    """step 4 in binary32 for a pixel that reads its own history with weight 1: returns (u, n, nu) after the last frame"""
    am = np.float32(alpha_min)
    for k, (rgb, gb, var) in enumerate(frames):
        d = np.where((gb[..., 10:11] > 0) & bool(flags), np.where(gb[..., :3] > eps, gb[..., :3], eps), np.float32(1))
        uc, nc = rgb / d, np.concatenate([var[..., :3] / (d * d), var[..., 3:]], -1)
        if k == 0:
            u, nu, n = uc, nc, np.ones(rgb.shape[:2] + (1,), np.float32)
            continue
        n1 = n + np.float32(1)
        a = np.maximum(np.float32(1) / n1, am)
        kk = np.float32(1) - a
        new = a < 1
        u, nu, n = np.where(new, kk * u + a * uc, uc), np.where(new, (kk * kk) * nu + (a * a) * nc, nc), np.where(new, n1, np.float32(1))
    return u, n[..., 0], nu


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("alpha_min", [0.0, 0.2, 1.0])
def test_equal_cameras_follow_the_recurrence(ftn, flags, alpha_min):
    """K frames of one camera whose G-buffer positions are jittered means and differ from frame to frame: motion is exactly zero, so every
    pixel, covered or not, reads its own history alone"""
    h, w, K = 37, 53, 6
    cam = R.pinhole((0.1, -0.2, -1.0), (w, h), 40.0, yaw=0.05, pitch=0.02)
    planes = [dict(z=4.0, xmax=1.5)]                                     # one plane (jitter cannot change what a pixel sees except at its
    frames = [R.make_frame(cam, planes, h, w, seed=k, jitter=0.0 if k == 0 else 0.3) for k in range(K)]   # edge), sky beside it
    same = np.all([f[1][..., 10] == frames[0][1][..., 10] for f in frames], axis=0)               # pixels of one coverage class throughout
    assert same.mean() > 0.95 and (frames[0][1][..., 10] == 0).any()
    p = dict(flags=flags, alpha_min=alpha_min, normal_tol=0.0, plane_tol=1e-5, albedo_tol=1.0)    # (the albedo moves with the jitter)
    hist = run_twin(ftn, [cam] * K, frames, p)[-1][0]
    u, n, nu = recurrence(frames, flags, alpha_min)
    for got, want in ((hist[..., :3], u), (hist[..., 3], n), (hist[..., 4:], nu)):
        assert np.array_equal(bits(got)[same], bits(want)[same])
    if alpha_min == 0.0:
        assert (hist[..., 3][same] == K).all()
        d = lambda f: np.where((f[1][..., 10:11] > 0) & bool(flags), np.maximum(f[1][..., :3].astype(np.float64), 1e-3), 1.0)
        want = sum(np.concatenate([f[2][..., :3].astype(np.float64) / d(f) ** 2, f[2][..., 3:]], -1) for f in frames) / K ** 2
        assert R.rel_error(hist[..., 4:][same], want[same]) <= 1e-5
    if alpha_min == 1.0:
        assert (hist[..., 3] == 1).all()


def silhouette_sequence(K=6, h=37, w=53):
    """K frames of one camera over TWO_PLANES: at the near plane's edge the jittered G-buffer sample falls on the near plane in one frame
    and on the far one in the next, as a renderer's mean over a few samples does at a silhouette"""
    cam = R.pinhole((0.1, -0.2, -1.0), (w, h), 40.0, yaw=0.05, pitch=0.02)
    return cam, [R.make_frame(cam, TWO_PLANES, h, w, seed=70 + k, jitter=0.45) for k in range(K)]


def test_equal_cameras_accumulate_across_a_silhouette(ftn):
    """Equal cameras look at the static scene alike, so a pixel's tap is the pixel itself and the two geometry tests are not made: a
    silhouette pixel whose G-buffer depth jumps by the planes' distance from frame to frame keeps its history at the default tolerances,
    follows the recurrence bit for bit and agrees with the restatement.  Under a camera moved by a hair the tests are made, and such a
    pixel is refused its own tap."""
    cam, frames = silhouette_sequence()
    K = len(frames)
    depth = np.stack([f[1][..., 9] for f in frames])
    same = np.all([f[1][..., 10] == frames[0][1][..., 10] for f in frames], axis=0)
    flips = same & (depth.max(0) - depth.min(0) > 1.0)
    assert flips.sum() >= 5
    p = dict(flags=0, alpha_min=0.0)

    def check(k, fr, c, prev, got):
        want = R.reference(*fr, c, (0, 0), prev, **p)
        assert not want[3].any()
        for g, x in zip(got, want[:3]):
            assert R.rel_error(g, x) <= TWIN_BOUND
    hist = run_twin(ftn, [cam] * K, frames, p, check=check)[-1][0]
    u, n, nu = recurrence(frames, 0, 0.0)
    for got, want in ((hist[..., :3], u), (hist[..., 3], n), (hist[..., 4:], nu)):
        assert np.array_equal(bits(got)[same], bits(want)[same])
    assert (hist[..., 3][same] == K).all()
    moved = R.pinhole((0.1 + 1e-4, -0.2, -1.0), cam["res"], 40.0, yaw=0.05, pitch=0.02)
    two = run_twin(ftn, [cam, moved], frames[:2], p)[-1][0]
    jump = np.abs(depth[1] - depth[0]) > 1.0
    assert jump.any() and (two[..., 3][jump] == 1).any() and (two[..., 3][~jump] == 2).mean() > 0.9


# ------------------------------------------------------------------ 4. no ghosting
def test_no_ghosting_across_a_depth_edge(ftn):
    """A red plane at distance 3 over x <= 0 in front of a blue one at distance 6, no noise, the camera moved sideways by 0.31: the
    near plane shifts by 8.27 pixels and the far one by 4.13.  No red reaches a far pixel, no blue a near one, and the far pixels the move
    revealed (every tap of theirs lands on the near plane of the previous frame, or outside it) start afresh."""
    h, w, f, dx = 64, 96, 80.0, 0.31
    planes = [dict(z=2.0, xmax=0.0, colour=(1.0, 0.0, 0.0)), dict(z=5.0, colour=(0.0, 0.0, 1.0))]
    cams = [R.pinhole((0.0, 0.0, -1.0), (w, h), f), R.pinhole((dx, 0.0, -1.0), (w, h), f)]
    frames = [R.make_frame(c, planes, h, w, sigma=0.0, jitter=0.0) for c in cams]
    assert all((fr[2] == 0).all() for fr in frames)
    # the analytic geometry, in pixel indices: a pixel of frame k shows the near plane when the ray through its centre meets z = 2 at x <= 0
    px = np.arange(w, dtype=np.float64)
    near = [(k * dx + (px + 0.5 - w / 2.0) * 3.0 / f) <= 0.0 for k in (0, 1)]
    s = px + f * dx / 6.0                                                # where a far pixel of frame 1 was in frame 0 (y does not move)
    i0 = np.floor(s).astype(int)
    assert np.abs(s - np.rint(s)).min() > 0.05                           # nothing borderline
    tap_bad = lambda i: (i >= w) | near[0][np.clip(i, 0, w - 1)]
    revealed = ~near[1] & tap_bad(i0) & tap_bad(i0 + 1)
    assert 3 <= (revealed & (px < w / 2)).sum() <= 5 and (revealed & (px > w - 8)).any()
    assert np.array_equal(frames[1][1][0, :, 9] < 4.0, near[1])          # the generated G-buffer agrees with it
    for flags in (0, 1):
        out = run_twin(ftn, cams, frames, dict(flags=flags, alpha_min=0.0, plane_tol=0.01, albedo_tol=1.0))[1]
        hist, rgb, var = out
        far = ~near[1]
        assert (rgb[:, far, 0] == 0).all() and (rgb[:, ~far, 2] == 0).all()
        assert (hist[:, revealed, 3] == 1).all() and (hist[:, far & ~revealed, 3] == 2).all()
        assert (var == 0).all()
        if flags == 0:
            assert np.array_equal(bits(rgb[:, revealed]), bits(frames[1][0][:, revealed]))
            assert np.array_equal(bits(rgb), bits(frames[1][0]))         # flat colours: accumulation changes nothing at all


# ------------------------------------------------------------------ 5. reprojection accuracy
def test_reprojection_stays_within_the_bilinear_error(ftn):
    """One plane at z = 3 facing a camera that does not turn, its colour the smooth texture(X) of _temporal_ref (second derivatives at most
    M = 0.4 k^2 = 0.9 in x and in y), no noise, the camera moved sideways, up and forward.  The plane is parallel to the image, so the
    previous frame's pixel centres are a square grid on it of spacing g = (distance / focal) = 4 / 100, and the history a pixel fetches is
    the bilinear interpolant of texture over that grid at the pixel's own surface point: off by at most g^2 / 8 (M + M) = 3.6e-4.
    With alpha = 1/2 the accumulated colour is off by half of that; 1e-5 is allowed for the binary32 arithmetic (values near 1)."""
    h, w, f = 64, 96, 100.0
    planes = [dict(z=3.0)]
    cams = [R.pinhole((0.0, 0.0, -1.0), (w, h), f), R.pinhole((0.13, -0.07, -0.8), (w, h), f)]
    frames = [R.make_frame(c, planes, h, w, sigma=0.0, jitter=0.0) for c in cams]
    hist, rgb, _ = run_twin(ftn, cams, frames, dict(flags=0, alpha_min=0.0))[1]
    g, M = 4.0 / f, 0.4 * 1.5 ** 2
    bound = 0.5 * g * g / 8.0 * (M + M) + 1e-5
    assert ((hist[..., 3] == 1) | (hist[..., 3] == 2)).all()
    # the pixels whose four taps all lie in the previous image (at its border the remaining taps are renormalised, which is no longer
    # bilinear interpolation): the previous camera sees the point X = (X.x, X.y, 3) at raster (w / 2, h / 2) + f X.xy / 4
    X = frames[1][1][..., 6:9].astype(np.float64)
    sx, sy = w / 2.0 + f * X[..., 0] / 4.0 - 0.5, h / 2.0 + f * X[..., 1] / 4.0 - 0.5           # in pixel indices
    two = (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
    assert two.mean() > 0.7 and (hist[..., 3][two] == 2).all()
    truth = R.texture(frames[1][1][..., 6:9].astype(np.float64))
    err = np.abs(rgb.astype(np.float64) - truth)
    print("reprojection: worst error %.3g of a bound of %.3g" % (err[two].max(), bound))
    assert err[two].max() <= bound
    assert err[two].max() >= 1e-6                                        # (the history did contribute)
    unmoved = np.abs(0.5 * (frames[0][0].astype(np.float64) + frames[1][0]) - truth)
    assert unmoved[two].max() > 50 * bound                               # without reprojection the blend would be far off


# ------------------------------------------------------------------ 6. edge inputs
def edge_case_inputs():
    """(cams, frames, prev history edits) of a 48 x 64 sequence with non-finite colours, NaN, negative and infinite variances, NaN and
    infinite positions in the second frame, and n = 0, NaN n and NaN colour in the first frame's history"""
    h, w = 48, 64
    cams, frames = sequence(h, w, 1.7, n=2, seed=77)
    rgb, gb, var = (a.copy() for a in frames[1])
    rgb[10, 10] = (np.nan, 0.2, 0.3)
    rgb[20, 30] = (np.inf, 1.0, 1.0)
    rgb[21, 31, 2] = -np.inf
    var[12, 12, 0] = np.nan
    var[14, 40, 1] = -1e-3
    var[15, 41, 3] = -1e-3
    var[16, 42, 3] = np.nan
    var[30:34, 30:34] = np.inf
    var[36, 20, 1] = np.inf
    gb[5, 40, 6] = np.nan
    gb[25, 20, 7] = np.inf
    gb[26, 21, 3] = np.nan
    return cams, [frames[0], (rgb, gb, var)]


def spoil_history(hist):
    hist = hist.copy()
    hist[8:12, 20:24, 3] = 0.0
    hist[28, 8:12, 3] = np.nan
    hist[40, 30:34, 0] = np.nan
    hist[41, 30:34, 5] = np.nan
    hist[42, 30:34, 1] = np.inf
    hist[43, 30:34, 6] = np.inf
    return hist


def test_edge_inputs(ftn):
    cams, frames = edge_case_inputs()
    h, w = frames[0][0].shape[:2]
    film = R.film_desc(A, (w, h))
    for flags in (0, 1):
        p = dict(flags=flags, normal_tol=0.05, plane_tol=0.004)
        first = T.temporal_accumulate_cpu(ftn, *frames[0], R.camera_desc(A, cams[0]), film, None, p)
        hist0 = spoil_history(first[0])
        rgb, gb, var = frames[1]
        got = T.temporal_accumulate_cpu(ftn, rgb, gb, var, R.camera_desc(A, cams[1]), film, (R.camera_desc(A, cams[0]), frames[0][1], hist0), p)
        want = R.reference(rgb, gb, var, cams[1], (0, 0), (cams[0], frames[0][1], hist0), **p)
        ok = ~want[3]
        assert (~ok).mean() <= 0.02
        for g, x in zip(got, want[:3]):
            assert R.rel_error(g[ok], x[ok]) <= TWIN_BOUND
        hist, out, ovar = got
        for y, x in ((10, 10), (20, 30), (21, 31), (12, 12), (14, 40), (15, 41), (16, 42)):     # pass-through: copied, and no history kept
            assert np.array_equal(bits(out[y, x]), bits(rgb[y, x])) and np.array_equal(bits(ovar[y, x]), bits(var[y, x])), (y, x)
            assert (bits(hist[y, x]) == 0).all()
        assert np.isinf(ovar[30:34, 30:34]).all() and (hist[30:34, 30:34, 3] >= 1).all()       # unknown variance stays unknown, and usable
        assert np.isinf(ovar[36, 20, 1]) and np.isfinite(ovar[36, 20, [0, 2, 3]]).all()
        assert hist[5, 40, 3] == 1 and hist[25, 20, 3] == 1 and hist[26, 21, 3] == 1            # motion or features not finite: no history
        usable = hist[..., 3] > 0
        assert np.isfinite(hist[..., :3][usable]).all() and not np.isnan(hist[usable]).any()    # spoiled history never spreads
        assert np.isfinite(out[usable]).all()


def test_no_history_cases(ftn):
    """motion that leaves the image, a surface behind the previous camera, alpha_min = 1: every pixel starts afresh"""
    h, w = 9, 17
    planes = [dict(z=2.0)]
    cur = R.pinhole((0, 0, -1.0), (w, h), 12.0)
    fr = R.make_frame(cur, planes, h, w, seed=1)
    film = R.film_desc(A, (w, h))
    ones = np.ones((h, w, 8), np.float32)
    for prev_cam in (R.pinhole((40.0, 0, -1.0), (w, h), 12.0),           # far to the side
                     R.pinhole((0, 0, 10.0), (w, h), 12.0),              # beyond the plane, looking away from it
                     R.pinhole((0, 0, 2.0), (w, h), 12.0)):              # in the plane: depth 0, the projection divides by zero
        hist, out, ovar = T.temporal_accumulate_cpu(ftn, *fr, R.camera_desc(A, cur), film, (R.camera_desc(A, prev_cam), fr[1], ones), dict(flags=0))
        assert (hist[..., 3] == 1).all() and np.array_equal(bits(out), bits(fr[0])) and np.array_equal(bits(ovar), bits(fr[2]))
    hist, out, _ = T.temporal_accumulate_cpu(ftn, *fr, R.camera_desc(A, cur), film, (R.camera_desc(A, cur), fr[1], ones), dict(flags=0, alpha_min=1.0))
    assert (hist[..., 3] == 1).all() and np.array_equal(bits(out), bits(fr[0]))
    hist, _, _ = T.temporal_accumulate_cpu(ftn, *fr, R.camera_desc(A, cur), film, (R.camera_desc(A, cur), fr[1], ones), dict(flags=0, alpha_min=0.0))
    assert (hist[..., 3] == 2).all()


@pytest.mark.parametrize("h,w", [(1, 1), (1, 40), (40, 1)])
def test_thin_images(ftn, h, w):
    cams = [R.pinhole((0, 0, -1.0), (w, h), 30.0), R.pinhole((0.1, 0.1, -1.0), (w, h), 30.0, yaw=0.01)]
    frames = [R.make_frame(c, TWO_PLANES, h, w, seed=k) for k, c in enumerate(cams)]
    p = dict(alpha_min=0.0)

    def check(k, fr, cam, prev, got):
        want = R.reference(*fr, cam, (0, 0), prev, **p)
        ok = ~want[3]
        for g, x in zip(got, want[:3]):
            assert R.rel_error(g[ok], x[ok]) <= TWIN_BOUND
    out = run_twin(ftn, cams, frames, p, check=check)
    if h == 1 and w == 1:                                                # a shift of 1 pixel and more: the one pixel finds nothing
        assert out[1][0][0, 0, 3] == 1
    out = run_twin(ftn, [cams[0]] * 2, frames[:1] * 2, p)                # equal cameras: every pixel finds itself
    assert (out[1][0][..., 3] == 2).all()


def test_uncovered_pixels_under_a_pure_rotation(ftn):
    """nothing but sky, the camera turned by 2.3 pixels: every pixel reprojects by its direction, and the sky accumulates"""
    h, w, f = 48, 64, 50.0
    cams = [R.pinhole((0, 0, 0), (w, h), f), R.pinhole((0, 0, 0), (w, h), f, yaw=2.3 / f, pitch=0.6 / f)]
    frames = [R.make_frame(c, [], h, w, seed=k) for k, c in enumerate(cams)]
    assert all((fr[1][..., 10] == 0).all() for fr in frames)
    p = dict(alpha_min=0.0)
    got = run_twin(ftn, cams, frames, p)[1]
    want = R.reference(*frames[1], cams[1], (0, 0), (cams[0], frames[0][1], run_twin(ftn, cams[:1], frames[:1], p)[0][0]), **p)
    ok = ~want[3]
    for g, x in zip(got, want[:3]):
        assert R.rel_error(g[ok], x[ok]) <= TWIN_BOUND
    n = got[0][..., 3]
    assert (n[4:-4, 4:-4] == 2).all() and (n == 1).any()                 # the interior finds history, the edge the turn brought in does not
    moved = run_twin(ftn, [cams[0], R.pinhole((5.0, -3.0, 1.0), (w, h), f)], frames, p)[1]       # a translation does not move the sky
    assert (moved[0][..., 3] == 2).all()


# ------------------------------------------------------------------ 7. threads
def test_result_does_not_depend_on_the_thread_count(ftn):
    cams, frames = sequence(640, 640, 2.3, n=2, seed=3)                  # 409,600 pixels: parallel_for uses up to 7 threads
    old = os.environ.get("FTN_BVH_THREADS")
    got = {}
    try:
        for nt in (1, 7):
            os.environ["FTN_BVH_THREADS"] = str(nt)
            got[nt] = run_twin(ftn, cams, frames, None)[1]
    finally:
        if old is None: os.environ.pop("FTN_BVH_THREADS", None)
        else: os.environ["FTN_BVH_THREADS"] = old
    for a, b in zip(got[1], got[7]):
        assert np.array_equal(bits(a), bits(b))
    assert (got[1][0][..., 3] == 2).mean() > 0.5
