"""The host side of the ambient-occlusion pass (include/fountain_hip_ao.h) without a GPU: ftn_ao_rays -- the code the kernel calls,
compiled for the host -- against the reference's rays bit for bit and against a float64 restatement; the distribution of its directions;
ftn_ao_resolve against a numpy float32 restatement bit for bit."""
import ctypes as C

import numpy as np
import pytest

from fountain_amd import ao as AO

import _ao_ref as AR
import _gbuffer_ref as GR

F32 = np.float32
U = 2.0 ** -24          # unit roundoff of binary32
bits = GR.bits


def _edge_draws(rng, n):
    """random pairs with the edge cases in front: components of 0, components just below 1, the centre of the disk"""
    one = float(np.nextafter(F32(1.0), F32(0.0)))
    edge = [(0.0, 0.0), (0.0, 0.5), (0.5, 0.0), (one, one), (one, 0.0), (0.0, one), (0.5, 0.5), (one, 0.5), (0.5, one), (0.25, 0.75)]
    u = rng.random((n, 2)).astype(F32)
    u[u >= 1.0] = one
    u[:len(edge)] = np.array(edge, F32)[:n]
    return u


@pytest.fixture(scope="module")
def records(orc_det):
    """interaction records of the oracle's intersect_full: the first surfaces of Cornell (triangles and two or three spheres) and of the
    rounded-cube fixture, 40 x 24 pixels at 2 spp each, and hand-made ones: normals with |x| == |y|, and normals facing away from wo"""
    recs = []
    for make in (AR.cornell, AR.rounded_cube):
        fs = AR.first_surfaces(orc_det, make, 2, 77, (0.0, 0.0, 1.0, 1.0), None)
        recs.append(fs["full"][fs["prim"] >= 0])
    rng = np.random.default_rng(11)
    hand = np.zeros((64, 24), F32)
    hand[:, 0:3] = rng.normal(size=(64, 3)) * 3
    hand[:, 3:6] = np.abs(rng.normal(size=(64, 3))) * 1e-6
    for i in range(64):
        a, c = rng.normal(), rng.normal()
        n = np.array([a, a if i % 2 else -a, c if i % 4 < 2 else 0.0])
        n /= np.linalg.norm(n)
        wo = rng.normal(size=3)
        wo /= np.linalg.norm(wo)
        if i % 3 == 0 and np.dot(n, wo) > 0:          # the surface seen from behind: the hemisphere stands on -n
            wo = -wo
        hand[i, 6:9], hand[i, 11:14] = n, wo
    assert (np.abs(hand[:, 6]) == np.abs(hand[:, 7])).all()
    assert ((hand[:, 6:9].astype(np.float64) * hand[:, 11:14]).sum(-1) < 0).sum() >= 16
    recs.append(hand)
    out = np.concatenate(recs)
    assert 2000 < len(out) < 8000 and (np.abs(out[:, 3:6]).sum(-1) > 0).all()
    return out


def test_rays_equal_the_reference_bit_for_bit(ftn, orc_det, records):
    rng = np.random.default_rng(3)
    u = _edge_draws(rng, len(records))
    for radius in (AR.INF, 0.75):
        got = AO.ao_rays(ftn, records, u, radius)
        want = np.array([AR.ao_ray_ref(orc_det, records[i], u[i], radius) for i in range(len(records))], F32)
        bad = (bits(got) != bits(want)).any(-1)
        assert not bad.any(), "%d of %d rays differ, first %d: %r vs %r" % (bad.sum(), len(bad), np.argmax(bad), got[np.argmax(bad)], want[np.argmax(bad)])
    # the same edge draws on the records that face away, and on those with |n.x| == |n.y|
    hand = records[-64:]
    for e in _edge_draws(rng, 10):
        uu = np.tile(e, (64, 1))
        got = AO.ao_rays(ftn, hand, uu)
        want = np.array([AR.ao_ray_ref(orc_det, hand[i], uu[i]) for i in range(64)], F32)
        assert np.array_equal(bits(got), bits(want)), e
    assert AO.ao_rays(ftn, np.zeros((0, 24), F32), np.zeros((0, 2), F32)).shape == (0, 8)


def test_directions_against_a_float64_restatement(ftn, orc_det, records):
    """d against the same construction in float64 from the float32 inputs (nf, the oracle's l): the frame normalised and crossed in
    float64.  Bounds, u = 2^-24: every float32 frame vector carries at most 3 roundings per component on top of nf's own (|s - s64|,
    |t - t64| <= 8 u), l enters exactly, and the combination rounds 5 times per component, so |d - d64| <= (8 + 8 + 2.5) u < 24 u per
    component and | |d| - 1 | <= 32 u = 16 ulps of 1 with nf's own length error (<= 3 u) included.  dot(d, nf) = l.z |nf|^2 up to the frame's
    departure from orthogonality, so it is at least l.z (1 - 8 u) - 16 u: non-negative for every l.z above 2^-20, and never below the
    rounding of an exact zero."""
    rng = np.random.default_rng(4)
    u = _edge_draws(rng, len(records))
    got = AO.ao_rays(ftn, records, u)
    worst_len, worst_d, worst_dot = 0.0, 0.0, 0.0
    for i in range(len(records)):
        nf, l, _ = AR.ao_direction(orc_det, records[i, 6:9], records[i, 11:14], u[i])
        nf64, l64 = nf.astype(np.float64), l.astype(np.float64)
        if abs(nf64[0]) > abs(nf64[1]):
            s = np.array([-nf64[2], 0.0, nf64[0]])
        else:
            s = np.array([0.0, nf64[2], -nf64[1]])
        s /= np.linalg.norm(s)
        t = np.cross(nf64, s)
        d64 = s * l64[0] + t * l64[1] + nf64 * l64[2]
        d = got[i, 3:6].astype(np.float64)
        worst_d = max(worst_d, np.abs(d - d64).max())
        worst_len = max(worst_len, abs(np.linalg.norm(d) - 1.0))
        dn = float(np.dot(d, nf64))
        worst_dot = min(worst_dot, dn - l64[2])
        assert dn >= l64[2] * (1 - 8 * U) - 16 * U, (i, dn, l64[2])
        if l64[2] > 2.0 ** -20:
            assert dn >= 0.0
    print("max |d - d64| %.3g (bound %.3g), max ||d| - 1| %.3g (bound %.3g), min dot(d, nf) - l.z %.3g" % (worst_d, 24 * U, worst_len, 32 * U, worst_dot))
    assert worst_d <= 24 * U and worst_len <= 32 * U


def test_directions_are_cosine_distributed(ftn):
    """over 10^5 stratified draws (a 400 x 250 grid, one jittered draw per cell) on a surface whose frame is the axes (n = wo = +z, so
    d = (-l.y, l.x, l.z) exactly): E[l.z] = 2/3 and E[l.z^2] = 1/2 for p(w) = cos / pi.  Margins: four standard errors of 10^5
    independent draws (stratifying only lowers the error): Var l.z = 1/2 - 4/9 = 1/18, Var l.z^2 = 1/3 - 1/4 = 1/12."""
    nx, ny = 400, 250
    n = nx * ny
    rng = np.random.default_rng(9)
    gx, gy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    u = np.stack([(gx.ravel() + rng.random(n)) / nx, (gy.ravel() + rng.random(n)) / ny], -1).astype(F32)
    u[u >= 1.0] = np.nextafter(F32(1.0), F32(0.0))
    rec = np.zeros((n, 24), F32)
    rec[:, 3:6], rec[:, 8], rec[:, 13] = 1e-7, 1.0, 1.0
    r = AO.ao_rays(ftn, rec, u)
    z = r[:, 5].astype(np.float64)
    assert (z >= 0).all() and np.array_equal(r[:, 6], np.full(n, np.inf, F32)) and not r[:, 7].any()
    assert (r[:, 2] > 0).all() and np.allclose(r[:, 0:2], 0, atol=1e-6)          # origins offset off the surface, along +z only
    m1, m2 = z.mean(), (z * z).mean()
    se1, se2 = np.sqrt(1 / 18 / n), np.sqrt(1 / 12 / n)
    print("mean l.z %.6f (2/3 +- %.2g), mean l.z^2 %.6f (1/2 +- %.2g)" % (m1, 4 * se1, m2, 4 * se2))
    assert abs(m1 - 2 / 3) <= 4 * se1 and abs(m2 - 0.5) <= 4 * se2
    # the azimuth is uniform: the first two components average to zero (Var = 1/4 each)
    assert np.abs(r[:, 3:5].astype(np.float64).mean(0)).max() <= 4 * np.sqrt(0.25 / n)


@pytest.mark.parametrize("rays", [1, 3, 64])
def test_resolve_equals_the_restatement_bit_for_bit(ftn, rays):
    raw = AR.synthetic_sums()
    got = AO.resolve(ftn, raw, rays)
    out = np.concatenate([got[k] for k in AO.CHANNELS], axis=-1)
    want = AR.resolve_ref(raw, rays)
    assert np.array_equal(bits(out), bits(want)), np.argwhere(bits(out) != bits(want))[:4]
    assert not out[0].any()                                             # weight == 0
    assert out[1].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 5.0]            # hit_weight == 0
    assert out[2].tolist() == [0.0, 0.0, 0.0, 0.0, 0.75, 4.0]           # every ray occluded
    assert out[5, 1:4].tolist() == [0.0, 0.0, 0.0]                      # a length that underflows
    assert np.isfinite(out).all()
