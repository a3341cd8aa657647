"""The host twins of include/fountain_hip_motion.h without a GPU: ftn_temporal_accumulate_motion_cpu and ftn_motion_vectors_cpu against
the float64 restatement of tests/_motion_ref.py on random inputs and on the edge rows; the two exact reductions to the existing call; the
motion of a translation parallel to the image plane against a binary64 projection, within a margin counted from project's binary32
operations; and, on synthetic frames of a square moving over a background, the orderings the stage exists for.  CPU only."""
import ctypes as C

import numpy as np
import pytest

from fountain_amd import _abi as A
from fountain_amd import motion as M
from fountain_amd import temporal as T

import _motion_ref as MR
import _temporal_ref as R
import test_temporal_cpu as TC          # its sequences and its twin-against-restatement margin: the arithmetic compared is the same

EPS32 = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def disturbed_mv8(gb, cam, rng):
    """gb12's own positions and normals, then per region what a moving scene and a careless caller give: an in-plane shift of a few pixels
    (history is fetched elsewhere and passes the tests), a shift off the plane (the plane test refuses), a turned normal, NaN, a point
    behind the previous camera, the other coverage class; the pixels along the border keep shifts that push taps over it"""
    h, w = gb.shape[:2]
    mv = MR.mv8_from_gb(gb)
    ys, xs = np.mgrid[0:h, 0:w]
    zone = (3 * ys // max(h, 1)) * 3 + (3 * xs // max(w, 1))            # 9 zones
    cov = gb[..., 10] > 0
    shift = rng.uniform(-0.25, 0.25, (h, w, 3)).astype(np.float32)
    shift[..., 2] = 0.0
    mv[..., 0:3] += np.where(((zone % 2 == 0) & cov)[..., None], shift, 0.0)
    mv[..., 2] += np.where((zone == 1) & cov, 0.05, 0.0).astype(np.float32)
    turn = (zone == 3) & cov
    mv[..., 3] = np.where(turn, mv[..., 3] + rng.uniform(-0.3, 0.3, (h, w)).astype(np.float32), mv[..., 3])
    pick = rng.uniform(size=(h, w))
    mv[..., 0] = np.where(pick < 0.01, np.nan, mv[..., 0])
    mv[..., 2] = np.where((pick >= 0.01) & (pick < 0.02), cam["eye"][2] - 1.0, mv[..., 2])        # q.z <= 0
    mv[..., 6] = np.where((pick >= 0.02) & (pick < 0.04), np.where(cov, 0.0, 1.0), mv[..., 6])     # coverage mismatch
    return np.ascontiguousarray(mv, dtype=np.float32)


# ------------------------------------------------------------------ 1. twins against the restatement
def test_twins_against_restatement(ftn):
    """moving and equal cameras, both flags, a crop origin, with the edge rows in every frame: each frame of the twin against the
    restatement fed with the twin's own history; the motion vectors of the same inputs likewise"""
    tally = dict(pixels=0, fragile=0, worst=0.0, worst_mv=0.0, moved=0, rejected=0)
    for (h, w), motion, flags in (((3, 5), 0.3, 1), ((9, 17), 4.7, 0), ((48, 64), 0.3, 1), ((48, 64), 4.7, 0), ((48, 64), 0.0, 1), ((1, 1), 0.3, 0)):
        rng = np.random.default_rng(100 * h + w + flags)
        cams, frames = TC.sequence(h, w, motion, seed=7 * h + w)
        if motion == 0.0:
            cams = [cams[0]] * len(cams)                                  # equal cameras: the per-pixel shortcut
            frames = [R.make_frame(cams[0], TC.TWO_PLANES, h, w, seed=5 + k, normal_noise=0.1, jitter=0.0) for k in range(len(cams))]
        p = dict(flags=flags, alpha_min=0.2, normal_tol=0.05, plane_tol=0.004, albedo_tol=0.003)
        origin = (7, 3) if flags else (0, 0)
        film = R.film_desc(A, (w, h), origin, full=(w + origin[0] + 3, h + origin[1] + 2))
        prev, prev_ref = None, None
        for k, (cam, fr) in enumerate(zip(cams, frames)):
            mv8 = disturbed_mv8(fr[1], cam, rng)
            got = T.temporal_accumulate_cpu(ftn, *fr, R.camera_desc(A, cam), film, prev, p, motion=mv8)
            want = MR.reference_motion(*fr, cam, mv8, origin, prev_ref, **p)
            ok = ~want[3]
            tally["pixels"] += ok.size
            tally["fragile"] += int((~ok).sum())
            for g, x in zip(got, want[:3]):
                tally["worst"] = max(tally["worst"], R.rel_error(g[ok], x[ok]))
            if prev is not None:
                plain = T.temporal_accumulate_cpu(ftn, *fr, R.camera_desc(A, cam), film, prev, p)
                tally["moved"] += int((bits(plain[0]) != bits(got[0])).any(-1).sum())
                tally["rejected"] += int(((got[0][..., 3] == 1) & (plain[0][..., 3] > 1)).sum())
                mo = M.motion_vectors_cpu(ftn, mv8, fr[1], R.camera_desc(A, cam), prev[0], film)
                want_mo, frag = MR.motion_vectors(mv8, fr[1], cam, prev_ref[0], origin)
                assert np.array_equal(np.isnan(mo)[~frag], np.isnan(want_mo)[~frag])
                fin = ~np.isnan(want_mo) & ~frag[..., None]
                if fin.any():
                    tally["worst_mv"] = max(tally["worst_mv"], float(np.abs(mo[fin] - want_mo[fin]).max() / max(h, w)))
            prev, prev_ref = (R.camera_desc(A, cam), fr[1], got[0]), (cam, fr[1], got[0])
    print("motion twins against restatement: worst relative error %.3g, motion vectors %.3g of the image, %d of %d pixels fragile; mv8 changed %d "
          "pixels and refused %d their history" % (tally["worst"], tally["worst_mv"], tally["fragile"], tally["pixels"], tally["moved"], tally["rejected"]))
    assert tally["moved"] > 1000 and tally["rejected"] > 50            # the inputs exercise what they are meant to
    assert tally["fragile"] <= TC.FRAGILE_MAX * tally["pixels"]
    assert tally["worst"] <= TC.TWIN_BOUND
    assert tally["worst_mv"] <= 41 * EPS32                               # project's operation count: test_parallel_translation below


def test_edge_rows(ftn):
    """one frame, pixel by pixel: NaN, uncovered, q.z <= 0, coverage mismatch and a tap pushed over the border"""
    h, w = 4, 6
    cam = R.pinhole((0, 0, 0), (w, h), 4.0)
    pcam = R.pinhole((0.1, 0, 0), (w, h), 4.0)
    fr0 = R.make_frame(pcam, [dict(z=3.0)], h, w, seed=1, jitter=0.0)
    fr1 = R.make_frame(cam, [dict(z=3.0)], h, w, seed=2, jitter=0.0)
    fr1[1][0, :, :] = 0.0                                               # row 0: uncovered
    fr1[1][0, :, 11] = 4.0
    film = R.film_desc(A, (w, h))
    p = dict(flags=0, alpha_min=0.0, normal_tol=0.05, plane_tol=0.004)          # (without demodulation a pixel without history is a copy)
    h0 = T.temporal_accumulate_cpu(ftn, *fr0, R.camera_desc(A, pcam), film, None, p)[0]
    prev = (R.camera_desc(A, pcam), fr0[1], h0)
    mv = MR.mv8_from_gb(fr1[1])
    mv[1, 0, 0] = np.nan                                                # NaN position
    mv[1, 1, 2] = -1.0                                                  # behind the previous camera
    mv[1, 2, 6] = 0.0                                                   # coverage mismatch, covered pixel
    mv[0, 3, 6] = 1.0                                                   # coverage mismatch, uncovered pixel
    mv[2, 0, 0] -= 3.0 * 0.7 / 4.0                                      # 0.7 pixel (and the camera's 0.13) to the left of column 0: taps at -1 and 0
    mv[3, 5, 0] += 3.0 * 2.0 / 4.0                                      # two pixels right of the last column: outside
    hist, rgb, var = T.temporal_accumulate_cpu(ftn, *fr1, R.camera_desc(A, cam), film, prev, p, motion=mv)
    n = hist[..., 3]
    for y, x in ((1, 0), (1, 1), (1, 2), (0, 3), (3, 5)):
        assert n[y, x] == 1 and np.array_equal(bits(rgb[y, x]), bits(fr1[0][y, x])), (y, x)
    assert n[2, 0] == 2 and n[2, 3] == 2 and n[3, 4] == 2               # the border tap alone, and untouched neighbours, find history
    assert (n[0, :3] == 1).all()                                        # uncovered now, covered before: the other class
    mo = M.motion_vectors_cpu(ftn, mv, fr1[1], R.camera_desc(A, cam), prev[0], film)
    for y, x in ((1, 0), (1, 1), (1, 2), (0, 3)):
        assert np.isnan(mo[y, x]).all(), (y, x)
    assert np.isfinite(mo[0, :3]).all() and np.isfinite(mo[2:]).all()
    want, _ = MR.motion_vectors(mv, fr1[1], cam, pcam)
    assert np.allclose(mo[2:], want[2:], atol=41 * EPS32 * w, rtol=0)


# ------------------------------------------------------------------ 2. the exact reductions
@pytest.mark.parametrize("motion", [0.0, 0.3, 4.7])
def test_reductions_to_the_existing_call(ftn, motion):
    """a null mv8, and an mv8 copied from gb12, give the bits of ftn_temporal_accumulate_cpu: moving cameras and equal ones, NaN and
    uncovered pixels among them"""
    from fountain_amd.motion import _lib
    lib = _lib(ftn)
    h, w = 33, 47
    cams, frames = TC.sequence(h, w, motion or 1.0, seed=3)
    if motion == 0.0:
        cams = [cams[0]] * len(cams)
    film = R.film_desc(A, (w, h))
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    for flags in (0, 1):
        p = T.temporal_params(ftn, flags=flags, alpha_min=0.1, normal_tol=0.05, plane_tol=0.004)
        prev = None
        for k, (cam, fr) in enumerate(zip(cams, frames)):
            fr = [a.copy() for a in fr]
            fr[1][2, 3, 6] = np.nan                                    # a NaN position: its copy counts as the pixel's own
            fr[1][4, 5, 3:6] = -0.0
            fr[0][6, 7, 0] = np.inf                                     # a pixel that passes through
            cd = R.camera_desc(A, cam)
            want = T.temporal_accumulate_cpu(ftn, *fr, cd, film, prev, p)
            copied = T.temporal_accumulate_cpu(ftn, *fr, cd, film, prev, p, motion=MR.mv8_from_gb(fr[1]))
            for g, x in zip(copied, want):
                assert np.array_equal(bits(g), bits(x)), (motion, flags, k)
            hist, out, ovar = np.empty((h, w, 8), np.float32), np.empty((h, w, 3), np.float32), np.empty((h, w, 4), np.float32)
            pc, pg, ph = (C.byref(prev[0]), ptr(prev[1]), ptr(prev[2])) if prev else (None, None, None)
            assert lib.ftn_temporal_accumulate_motion_cpu(ptr(fr[0]), ptr(fr[1]), ptr(fr[2]), None, C.byref(cd), C.byref(film), w, h, pc, pg, ph, C.byref(p),
                                                          ptr(hist), ptr(out), ptr(ovar)) == 0
            for g, x in zip((hist, out, ovar), want):
                assert np.array_equal(bits(g), bits(x)), (motion, flags, k)
            prev = (cd, fr[1], want[0])
        assert (want[0][..., 3] > 1).mean() > 0.5                       # (most pixels did find history)


# ------------------------------------------------------------------ 3. a translation parallel to the image plane
def test_parallel_translation(ftn):
    """A plane z = 3 that moved by (dx, dy, 0) under a pinhole camera at the origin: the motion is -f (dx, dy) / z, and the twin agrees
    with a binary64 projection of the same binary32 inputs within the roundings of project.  Their count, per projection: m4_point with
    camera_to_world.inv rounds every component's sum 4 times at most (a product and three sums), its w as often, then the reciprocal
    and the product by it: (1 + e)^10; m4_point with raster_to_camera.inv the same on top: (1 + e)^20, relative to the sum of the terms'
    sizes, which for a point inside the image is at most f |x / z| + w / 2 <= w (the eye at the origin: no cancellation in the first
    product).  Two projections and the subtraction: 41 e w, e = 2^-24, first order (the second order is 1e-6 of that)."""
    h, w, f, z = 48, 64, 48.0, 3.0
    cam = R.pinhole((0, 0, 0), (w, h), f)
    rgb, gb, var = R.make_frame(cam, [dict(z=z)], h, w, seed=4, jitter=0.3)
    film, cd = R.film_desc(A, (w, h)), R.camera_desc(A, cam)
    worst = 0.0
    for dx, dy in ((0.25, 0.0), (-0.1, 0.3), (1e-3, -2e-3), (0.0, 0.0)):
        mv = MR.mv8_from_gb(gb)
        mv[..., 0] -= np.float32(dx)
        mv[..., 1] -= np.float32(dy)
        got = M.motion_vectors_cpu(ftn, mv, gb, cd, cd, film)
        want, _ = MR.motion_vectors(mv, gb, cam, cam)
        bound = 41 * EPS32 * w
        err = float(np.abs(got - want).max())
        worst = max(worst, err / bound)
        assert err <= bound, (dx, dy, err, bound)
        # the closed form, from inputs that are themselves rounded to binary32: x, x - d and z each within e of their value moves a
        # coordinate of size <= w / 2 by e w / 2: 3 more e w / 2
        exact = -f * np.array([dx, dy]) / z
        assert np.abs(got - exact).max() <= bound + 1.5 * EPS32 * w + f / z * EPS32 * 2, (dx, dy)
        if dx == 0.0 and dy == 0.0:
            assert (bits(got) == 0).all()                               # the same function on the same input: exactly zero
    print("parallel translation: worst error %.3g of the bound 41 e w" % worst)


# ------------------------------------------------------------------ 4. a square that moves over a background
def test_moving_square_orderings(ftn):
    """K frames of a textured square that moves two pixels a frame under a camera that stands still.  On the object's pixels the
    motion-aware result is closer to the clean image than the static call's on the same frames, and closer than the frame alone; a sky
    pixel the square has just left (uncovered) never takes the square's history.  Only the orderings are asserted."""
    h, w, K = 48, 64, 6
    cam = R.pinhole((0.5, 0.2, 0.0), (w, h), 48.0)          # the square straddles the background's left edge: sky behind its left part
    cd, film = R.camera_desc(A, cam), R.film_desc(A, (w, h))
    step = (0.09, 0.05)
    p = dict(alpha_min=0.2)
    frames = [MR.moving_square_frame(cam, k, h, w, step=step, seed=11) for k in range(K)]
    prev_m = prev_s = None
    for k, (rgb, gb, var, mv, clean, obj) in enumerate(frames):
        hm, om, _ = T.temporal_accumulate_cpu(ftn, rgb, gb, var, cd, film, prev_m, p, motion=mv if k else None)
        hs, os_, _ = T.temporal_accumulate_cpu(ftn, rgb, gb, var, cd, film, prev_s, p)
        prev_m, prev_s = (cd, gb, hm), (cd, gb, hs)
        if k:
            left = frames[k - 1][5] & ~(gb[..., 10] > 0)                 # the square was here, the sky is here now
            assert left.sum() > 5
            assert (hm[left][:, 3] == 1).all() and np.array_equal(bits(om[left]), bits(rgb[left]))
    inner = obj & frames[K - 2][5]                                        # (object pixels: all of them, the freshly covered rim included)
    rms = lambda a, m: float(np.sqrt(((a[m].astype(np.float64) - clean[m]) ** 2).mean()))
    e_motion, e_static, e_single = rms(om, obj), rms(os_, obj), rms(rgb, obj)
    print("moving square, %d frames, %d object pixels: rms error motion-aware %.4f, static %.4f, single frame %.4f (ratios %.2f and %.2f); mean history "
          "length on the object %.2f" % (K, int(obj.sum()), e_motion, e_static, e_single, e_static / e_motion, e_single / e_motion, float(hm[obj][:, 3].mean())))
    assert inner.sum() > 100
    assert e_motion < e_static and e_motion < e_single
