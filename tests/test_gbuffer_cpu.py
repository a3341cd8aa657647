"""The G-buffer's CPU pieces against independent restatements (tests/_gbuffer_ref.py): ftn_gbuffer_resolve bit for bit on hand-made
edge sums and on reconstructed buffers with misses, partial coverage and uncovered pixels; the oracle's camera ray differential and
texture differentials against a closed form.  CPU only."""
import ctypes as C

import numpy as np
import pytest

from fountain_amd import PerspectiveCamera
from fountain_amd import gbuffer as G

import _gbuffer_ref as GR

F32 = np.float32
bits = GR.bits


def _resolve(ftn, raw):
    r = G.resolve(ftn, raw)
    return np.concatenate([r[k] for k in G.CHANNELS], axis=-1)


def test_resolve_equals_the_restatement_on_edge_sums(ftn):
    rng = np.random.default_rng(3)
    raw = (rng.standard_normal((40, 12)) * 3).astype(F32)
    raw[:, 11] = rng.integers(0, 9, 40).astype(F32)
    raw[:, 10] = np.minimum(rng.integers(0, 9, 40), raw[:, 11]).astype(F32)
    raw[0, 10:12] = 0.0                          # w = 0, h = 0
    raw[1, 10:12] = (0.0, 3.0)                   # h = 0: misses only
    raw[2, 10:12] = (2.0, 5.0)                   # partial coverage
    raw[3, 10:12] = (4.0, 4.0)
    raw[4, 10:12] = (0.0, 0.0); raw[4, :10] = 7.0    # w = 0 with stray sums
    raw[5, 10:12] = (1.0, 3.0); raw[5, 0] = np.float32(1e-40)      # a subnormal sum
    got = _resolve(ftn, raw)
    assert np.array_equal(bits(got), bits(GR.resolve_ref(raw)))
    assert not got[0].any() and not got[4].any()
    assert got[1, 9] == np.inf and not got[1, 6:9].any() and got[2, 10] == F32(0.4)


def test_resolve_equals_the_restatement_on_reconstructed_buffers(ftn, orc_det):
    """a sky (misses, depth inf), a wide filter (partial coverage at silhouettes) and every other tile (uncovered pixels, w = 0)"""
    ref = GR.reconstruct(ftn, orc_det, lambda be: GR.textured_floor(be, (40, 30)), 2, 4, (0.0, 0.0, 1.0, 1.0), (0, 2, 0), radius=(1.25, 1.25))
    raw = ref["acc"]
    h, w = raw[..., 10], raw[..., 11]
    assert (w == 0).any() and ((h == 0) & (w > 0)).any() and ((h > 0) & (h < w)).any() and ((h > 0) & (h == w)).any()
    assert np.array_equal(bits(_resolve(ftn, raw)), bits(GR.resolve_ref(raw)))


@pytest.mark.parametrize("spp", [1, 16, 37])
def test_camera_ray_differential_closed_form(orc_det, spp):
    """the centre sample of a pinhole camera facing the plane z = 0 head-on from height h, on a quad with dpdu = (2L, 0, 0) and
    dpdv = (0, 2L, 0).  One pixel is q = tan(fov / 2) / (min(res) / 2) in camera space per unit depth, so the differential direction is
    e = (q, 0, 1) / sqrt(1 + q^2); scaled by s = 1 / sqrt(spp) it is d + s (e - d), which meets the plane at h s q / (sqrt(1 + q^2)
    (1 - s) + s) off the hit: dudx = that / 2L, and likewise dvdy"""
    res, fov, height, L = (64, 48), 50.0, 2.5, 3.0
    cam = PerspectiveCamera.look_at(orc_det, (0.0, 0.0, height), (0.0, 0.0, 0.0), (0, 1, 0), res, fov=fov)
    q = np.tan(np.radians(fov / 2)) / (min(res) / 2)
    s = 1.0 / np.sqrt(spp)
    hit12 = [0, 0, 0, 0, 0, 1, 2 * L, 0, 0, 0, 2 * L, 0]
    sample = (res[0] / 2, res[1] / 2, 0.5, 0.5, 0.0)
    ray, td = GR.camera_ray_differential(orc_det, cam, sample, spp, hit12)
    assert np.allclose(ray[0], (0, 0, height)) and np.allclose(ray[1], (0, 0, -1), atol=1e-7)
    assert np.allclose(ray[2], ray[0], atol=1e-6) and np.allclose(ray[4], ray[0], atol=1e-6)    # a pinhole: the differentials start at the eye
    want = height * s * q / (np.sqrt(1 + q * q) * (1 - s) + s) / (2 * L)
    for k, (main, cross) in enumerate(((td[0], td[1]), (td[3], td[2]))):
        e = ray[3 + 2 * k].astype(np.float64) - ray[1]
        assert abs(np.linalg.norm(e) / (s * np.hypot(q / np.sqrt(1 + q * q), 1 - 1 / np.sqrt(1 + q * q))) - 1) <= 1e-4
        assert abs(abs(float(main)) / want - 1) <= 1e-4, (spp, k, float(main), want)
        assert abs(float(cross)) <= 1e-5 * want
    _, none = GR.camera_ray_differential(orc_det, cam, sample, spp)
    assert not none.any()


def test_spawn_ray_export(orc_det):
    """SurfaceHit::spawn_ray: the origin moves off the surface by n . |p_err| to the side of the direction, one more ulp outward"""
    out = (C.c_float * 8)()
    p, e, n = (1.0, 2.0, 0.0), (1e-6, 1e-6, 1e-6), (0.0, 0.0, 1.0)
    for d, sign in (((0.0, 0.0, -1.0), -1), ((0.3, 0.0, 1.0), 1)):
        orc_det.lib.orc_kat_spawn_ray((C.c_float * 3)(*p), (C.c_float * 3)(*e), (C.c_float * 3)(*n), (C.c_float * 3)(*d), out)
        o = np.array(out[:], F32)
        assert o[0] == F32(1.0) and o[1] == F32(2.0) and np.sign(o[2]) == sign and F32(1e-6) < abs(o[2]) <= np.nextafter(F32(1e-6), F32(1))
        assert np.array_equal(o[3:6], np.array(d, F32)) and o[6] == np.inf and o[7] == 0.0
