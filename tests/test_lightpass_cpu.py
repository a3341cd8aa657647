"""The host side of the light-group pass (include/fountain_hip_lightpass.h) without a GPU: ftn_lightpass_terms -- the code the kernel
calls, compiled for the host -- against a numpy restatement of the definition bit for bit, its rays against the oracle's spawn-ray
arithmetic bit for bit, its term against float64 closed forms; ftn_lightpass_resolve and ftn_lightpass_compose against restatements."""
import numpy as np
import pytest

from fountain_amd import lightpass as LP

import _ao_ref as AR
import _gbuffer_ref as GR
import _lightpass_ref as LR

F32 = np.float32
U = 2.0 ** -24          # unit roundoff of binary32
bits = GR.bits

# the largest relative error of e against the float64 closed forms below, as measured on the host, and the
# factor section 3.1 puts on a measured error
MEASURED_REL_ERR = 3.2e-7        # 3.17e-07 = 5.32 u
TOL = 4 * MEASURED_REL_ERR


@pytest.fixture(scope="module")
def rows(orc_det):
    """interaction records of the oracle's intersect_full -- the first surfaces of the scene with one light of every kind (triangles
    and a sphere) and of Cornell, 40 x 24 pixels at 1 spp -- each paired with the oracle's sample of every light of its scene at random
    draws: (hit24, light24, scene) per scene"""
    rng = np.random.default_rng(21)
    out = []
    for make in (LR.every_kind, AR.cornell):
        fs = AR.first_surfaces(orc_det, make, 1, 77, (0.0, 0.0, 1.0, 1.0), None)
        full = fs["full"][fs["prim"] >= 0]
        sc = fs["scene"]
        n_lights = sc.info()["n_lights"]
        hit, l24 = [], []
        for li in range(n_lights):
            u = rng.random((len(full), 2)).astype(F32)
            hit.append(full)
            l24.append(LR.light_rows(orc_det, sc, li, full, u))
        out.append((np.concatenate(hit), np.concatenate(l24), n_lights, fs))
    assert out[0][2] == 5 and out[1][2] == 2
    return out


def test_terms_equal_the_restatement_and_the_reference_rays_bit_for_bit(ftn, orc_det, rows):
    n_rays = n_back = n_dark = 0
    for hit, l24, n_lights, _ in rows:
        for group in (1, n_lights):
            e, rays = LP.terms(ftn, hit, l24, group)
            for i in range(len(hit)):
                want_e, traced = LR.term_ref(hit[i], l24[i], group)
                assert np.array_equal(bits(e[i]), bits(want_e)), (i, e[i], want_e)
                want_r = LR.ray_ref(orc_det, hit[i], l24[i]) if traced else np.zeros(8, F32)
                assert np.array_equal(bits(rays[i]), bits(want_r)), (i, rays[i], want_r)
                n_rays += traced
                n_back += bool(l24[i, 6] > 0 and l24[i, 0:3].any() and not traced)
                n_dark += bool(not (l24[i, 6] > 0 and l24[i, 0:3].any()))
    # the rows reach every branch: rays, lights behind the surface (or facing away from it), and samples without radiance
    assert n_rays > 2000 and n_back > 200 and n_dark > 20, (n_rays, n_back, n_dark)
    e, rays = LP.terms(ftn, np.zeros((0, 24), F32), np.zeros((0, 24), F32), 3)
    assert e.shape == (0, 3) and rays.shape == (0, 8)


def test_hand_made_branches(ftn):
    """each test of the definition alone, on one surface n = ns = +z seen from above"""
    hit = np.zeros((7, 24), F32)
    hit[:, 3:6], hit[:, 8], hit[:, 22], hit[:, 11:14] = 1e-7, 1.0, 1.0, (0.0, 0.6, 0.8)
    l = np.zeros((7, 24), F32)
    l[:, 0:3], l[:, 3:6], l[:, 6], l[:, 7:10] = (2.0, 3.0, 4.0), (0.6, 0.0, 0.8), 0.5, (3.0, 0.0, 4.0)
    l[1, 6] = 0.0                                   # pdf 0
    l[2, 0:3] = 0.0                                 # black radiance
    l[3, 3:6], l[3, 7:10] = (0.6, 0.0, -0.8), (3.0, 0.0, -4.0)          # the light below the surface
    hit[4, 11:14] = (0.0, 0.6, -0.8)                # the surface seen from below, the light above
    l[5, 6] = np.inf                                # e underflows to black: radiance * (cos / inf) = 0
    hit[6, 20:23] = (1.0, 0.0, 0.0); l[6, 3:6] = (0.0, 0.6, 0.8)        # wi at a right angle to the shading normal: c = 0
    e, rays = LP.terms(ftn, hit, l, 3)
    c = F32(F32(0.8) / F32(0.5))
    assert np.array_equal(e[0], (np.array([2, 3, 4], F32) * c).astype(F32) * F32(3.0))
    assert rays[0, 6] == F32(F32(1.0) - F32(0.0001)) and rays[0, 7] == 0 and rays[0, 2] > 0
    assert np.allclose(rays[0, 0:3] + rays[0, 3:6], (3.0, 0.0, 4.0), atol=1e-6)
    assert not e[1:].any() and not rays[1:].any()
    assert LP.terms(ftn, hit[:1], l[:1], 1)[0][0].tolist() == ((np.array([2, 3, 4], F32) * c).astype(F32)).tolist()


def test_terms_against_float64_closed_forms(ftn, orc_det):
    """over the plane z = 0 (n = ns = +z), in float64 from the float32 inputs: a point light of intensity I at height h >= 1 leaves
    e = n I h / r^3 (r the distance), a distant light of radiance L from direction w leaves e = n L w.z.  The incidence stays within 60
    degrees of the normal, so no row is fragile and none is left out.  The light samples are the oracle's."""
    from fountain_amd import SceneBuilder, scenes
    rng = np.random.default_rng(8)
    I, L = np.array([12.0, 10.0, 8.0], F32), np.array([1.5, 2.5, 2.0], F32)
    worst = 0.0
    for trial in range(6):
        h = F32(1.0 + 3.0 * rng.random())
        lp = np.array([rng.normal(), rng.normal(), h], F32)
        tilt = np.radians(58.0) * rng.random()
        az = 2 * np.pi * rng.random()
        frm = np.array([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)], F32)
        b = SceneBuilder(orc_det)
        b.light_source("point", I=tuple(I), from_=tuple(lp))
        b.light_source("distant", L=tuple(L), from_=tuple(frm), to=(0, 0, 0))
        b.material("matte")
        scenes._quad(b, (-50, -50, 0), (50, -50, 0), (50, 50, 0), (-50, 50, 0))
        sc = b.create_scene()
        n = 400
        reach = float(h) * np.tan(np.radians(59.0))
        rad, phi = reach * np.sqrt(rng.random(n)), 2 * np.pi * rng.random(n)
        hit = np.zeros((n, 24), F32)
        hit[:, 0], hit[:, 1] = lp[0] + rad * np.cos(phi), lp[1] + rad * np.sin(phi)
        hit[:, 3:6], hit[:, 8], hit[:, 22] = 1e-6, 1.0, 1.0
        wo = rng.normal(size=(n, 3)); wo[:, 2] = np.abs(wo[:, 2]) + 0.05
        hit[:, 11:14] = wo / np.linalg.norm(wo, axis=1, keepdims=True)
        u = rng.random((n, 2)).astype(F32)
        for li, group in ((0, 1), (0, 2), (1, 2), (1, 5)):
            l24 = LR.light_rows(orc_det, sc, li, hit, u)
            e, rays = LP.terms(ftn, hit, l24, group)
            assert (rays[:, 6] > 0).all()
            p64 = hit[:, 0:3].astype(np.float64)
            if li == 0:
                d = lp.astype(np.float64) - p64
                r = np.linalg.norm(d, axis=1)
                assert (d[:, 2] / r >= 0.5 - 1e-9).all()
                want = group * I.astype(np.float64)[None, :] * (d[:, 2] / r ** 3)[:, None]
            else:
                w = frm.astype(np.float64) / np.linalg.norm(frm.astype(np.float64))
                assert w[2] >= 0.5
                want = group * L.astype(np.float64)[None, :] * w[2] * np.ones((n, 1))
            rel = np.abs(e.astype(np.float64) - want) / want
            worst = max(worst, rel.max())
    print("largest relative error of e against the float64 closed forms: %.3g (%.2f u); tolerance %.3g" % (worst, worst / U, TOL))
    assert worst <= TOL


def test_resolve_equals_the_restatement(ftn):
    raw = LR.synthetic_sums()
    out = LP.resolve8(ftn, raw)
    want = LR.resolve_ref(raw)
    assert np.array_equal(bits(out), bits(want)), np.argwhere(bits(out) != bits(want))[:4]
    assert not out[0].any()                                                         # weight == 0
    assert out[1].tolist() == [0, 0, 0, 0, 0, 0, 1.0, 0.0]                          # hit_weight == 0
    assert out[2].tolist() == [0, 0, 0, 0, 0, 0, 1.0, 0.75]                         # Y(unshadowed) == 0
    assert out[3, 6] == 0.0 and out[4, 6] == 1.0 and out[6, 6] == 1.0
    assert np.isfinite(out).all()
    # against float64: every quotient is one correctly rounded divide of float32 sums; the luminances carry 5 roundings each
    want64 = LR.resolve_ref(raw, np.float64)
    got = {k: out[..., s] for k, s in LP.CHANNELS.items()}
    assert np.allclose(out[:, 0:6], want64[:, 0:6], rtol=U, atol=0) and np.allclose(out[:, 7], want64[:, 7], rtol=U, atol=0)
    ok = raw[:, 3:6].min(-1) > 1e-20
    assert np.allclose(out[ok, 6], want64[ok, 6], rtol=8 * U, atol=0)
    assert got["lit"].shape == (len(raw), 3) and got["visibility"].shape == (len(raw), 1)


def test_compose_equals_the_restatement_bit_for_bit(ftn):
    rng = np.random.default_rng(13)
    h, w = 9, 13
    gb = rng.random((h, w, 12)).astype(F32)
    gb[..., 10] = rng.integers(0, 3, (h, w)) / 2.0           # coverage 0, 0.5 or 1
    gb[0, 0, 0:3] = 0.0
    for groups in (1, 3, 16):
        res8 = (rng.random((groups, h, w, 8)) * 5).astype(F32)
        res8[0, 1, 1, 0:3] = 0.0
        gains = (rng.random((groups, 3)) * 3 - 0.5).astype(F32)
        got = LP.compose(ftn, gb, res8, gains)
        assert np.array_equal(bits(got), bits(LR.compose_ref(gb, res8, gains))), groups
        assert not got[gb[..., 10] == 0].any() and got[gb[..., 10] != 0].any()
    # one group, gains of 1: albedo * INV_PI * lit in that association
    res8 = (rng.random((1, h, w, 8)) * 5).astype(F32)
    got = LP.compose(ftn, gb, res8, np.ones((1, 3), F32))
    want = ((gb[..., 0:3] * LR.INV_PI).astype(F32) * res8[0, ..., 0:3]).astype(F32)
    want[gb[..., 10] == 0] = 0.0
    assert np.array_equal(bits(got), bits(want))
    with pytest.raises(ValueError):
        LP.compose(ftn, gb, res8, np.ones((2, 3), F32))
    with pytest.raises(ValueError):
        LP.compose(ftn, gb, res8[:, :-1], np.ones((1, 3), F32))


def test_groups(orc_det):
    """the index lists follow ftn_scene_get_lights' order; Scene.lights() is the oracle's twin of it"""
    b, _, _ = LR.every_kind(orc_det)
    sc = b.create_scene()
    assert sc.lights()[0].tolist() == [0, 1, 2, 3, 3]
    assert LP.groups(sc, "kind") == {"point": [0], "distant": [1], "infinite": [2], "area": [3, 4]}
    assert LP.groups(sc, "each") == {"light0": [0], "light1": [1], "light2": [2], "area": [3, 4]}
    b, _, _ = LR.open_floor(orc_det)
    assert LP.groups(b.create_scene(), "kind") == {"point": [0], "distant": [1]} and LP.groups(b.create_scene(), "each") == {"light0": [0], "light1": [1]}
    with pytest.raises(ValueError):
        LP.groups(sc, "colour")
