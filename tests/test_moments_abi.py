"""The second-moments extension of the C ABI (include/fountain_hip_moments.h) without a GPU: the header, the ctypes mirror and the
library's exports agree; the layout and versions; ftn_moments_resolve against a float32 numpy restatement, bit for bit; the refusals,
which come before any device work, and FTN_ERR_NO_DEVICE where there is no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fountain_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fountain_hip_moments.h")
F32 = np.float32


def moments_header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ftn_[a-z0-9_]+)\s*\(", src)))


def test_header_mirror_and_exports_agree(ftn):
    assert moments_header_functions() == sorted(A.MOMENTS_FUNCTIONS)
    for other in (A.DECLARED_FUNCTIONS, A.GBUFFER_FUNCTIONS, A.DENOISE_FUNCTIONS):
        assert not set(A.MOMENTS_FUNCTIONS) & set(other)
    for name in A.MOMENTS_FUNCTIONS:
        assert hasattr(ftn.lib, name), "libfountain_hip.so does not export %s" % name


def test_pixel_layout():
    assert C.sizeof(A.ftn_moment_pixel) == 16 == A.SIZES["ftn_moment_pixel"]
    offsets = {name: getattr(A.ftn_moment_pixel, name).offset for name, _ in A.ftn_moment_pixel._fields_}
    assert offsets == {"sq": 0, "sq_y": 12}


def test_versions(ftn):
    header = open(HEADER).read()
    assert int(re.search(r"#define\s+FTN_MOMENTS_ABI_VERSION\s+(\d+)", header).group(1)) == A.FTN_MOMENTS_ABI_VERSION == 1
    assert ftn.lib.ftn_moments_abi_version() == A.FTN_MOMENTS_ABI_VERSION
    assert ftn.lib.ftn_abi_version() == A.FTN_ABI_VERSION == 3          # the main ABI is unchanged by the extension


def resolve_ref(pix, m):
    """the header's resolve in float32, one rounding per step: S = xyz_to_rgb(xyz) (ftn_math.h, left to right) for r, g, b and xyz[1]
    for Y; W < 2 -> +inf; mean = S / W; v = sq / W - mean * mean; v < 0 -> 0; v / (W - 1)"""
    pix, m = np.asarray(pix, F32), np.asarray(m, F32)
    x, y, z, w = (pix[..., k] for k in range(4))
    with np.errstate(all="ignore"):
        r = F32(3.240479) * x - F32(1.537150) * y - F32(0.498535) * z
        g = F32(-0.969256) * x + F32(1.875991) * y + F32(0.041556) * z
        b = F32(0.055648) * x - F32(0.204043) * y + F32(1.057311) * z
        s = np.stack([r, g, b, y], axis=-1).astype(F32)
        W = w[..., None]
        mean = (s / W).astype(F32)
        v = (m / W).astype(F32) - (mean * mean).astype(F32)
        v = np.where(v < 0, F32(0), v).astype(F32)
        out = (v / (W - F32(1))).astype(F32)
    out[w < 2] = np.inf
    return out


def _resolve(ftn, pix, m):
    pix, m = np.ascontiguousarray(pix, F32), np.ascontiguousarray(m, F32)
    out = np.full(pix.shape, np.nan, F32)
    ftn.check(ftn.lib.ftn_moments_resolve(pix.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), C.c_size_t(pix.size // 4),
                                          out.ctypes.data_as(C.c_void_p)))
    return out


def test_resolve_bits(ftn):
    rng = np.random.default_rng(11)
    n = 4096
    L = rng.uniform(0.0, 4.0, (n, 8, 3)).astype(F32)                           # 8 samples per pixel, rgb radiance
    xyz = np.stack([F32(0.412453) * L[..., 0] + F32(0.357580) * L[..., 1] + F32(0.180423) * L[..., 2],
                    F32(0.212671) * L[..., 0] + F32(0.715160) * L[..., 1] + F32(0.072169) * L[..., 2],
                    F32(0.019334) * L[..., 0] + F32(0.119193) * L[..., 1] + F32(0.950227) * L[..., 2]], -1).astype(F32)
    pix = np.concatenate([xyz.sum(1, dtype=F32), np.full((n, 1), 8, F32)], -1).astype(F32)
    m = np.concatenate([(L * L).sum(1, dtype=F32), (xyz[..., 1:2] ** 2).sum(1, dtype=F32)], -1).astype(F32)
    # the edges: W = 0, 1, 2, 2^24; cancellation below zero (clamped to 0); NaN and inf in every input
    pix[0] = [0, 0, 0, 0]
    pix[1, 3] = 1.0
    pix[2, 3] = 2.0
    pix[3] = [3.0 * 2 ** 24, 2.0 ** 24, 1.0, 2.0 ** 24]
    m[3] = [1.0, 1.0, 1.0, 1.0]
    pix[4] = [0.0, 9.0, 0.0, 3.0]
    m[4, 3] = F32(27.0) * (1 - F32(2.0 ** -20))                                # sq / W just below mean^2: negative, clamps to 0
    pix[5, 0] = np.nan
    m[6, 1] = np.nan
    pix[7, 3] = np.nan
    m[8, 2] = np.inf
    pix[9, 1] = np.inf
    pix[10, 3] = np.inf
    pix[11, 3] = F32(2.0) - F32(2.0 ** -23)                                   # just below 2: still +inf
    out = _resolve(ftn, pix, m)
    want = resolve_ref(pix, m)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert np.isinf(out[0]).all() and np.isinf(out[1]).all() and np.isinf(out[11]).all() and np.isfinite(out[2]).all()
    assert out[4, 3] == 0.0 and np.isnan(out[5, :3]).all() and np.isnan(out[6, 1]) and np.isnan(out[7]).all()
    assert np.isfinite(out[3]).all() and (out[3] >= 0).all()
    # the estimate on ordinary pixels: the sample variance of the 8 values over 8
    ok = slice(16, None)
    y = xyz[ok, :, 1].astype(np.float64)
    assert np.allclose(out[ok, 3], y.var(1, ddof=1) / 8, rtol=1e-3, atol=1e-6)
    assert ftn.lib.ftn_moments_resolve(None, m.ctypes.data_as(C.c_void_p), C.c_size_t(1), out.ctypes.data_as(C.c_void_p)) == A.FTN_ERR_INVALID_ARGUMENT
    assert ftn.lib.ftn_moments_resolve(None, None, C.c_size_t(0), None) == A.FTN_OK


def _args(ftn, integrator=None, sampler=None, pipeline=A.FTN_PIPELINE_AUTO):
    from fountain_amd import PathIntegrator, PerspectiveCamera, RandomSampler, Film, Transform
    cam = PerspectiveCamera(ftn, Transform.identity(ftn), (8, 8))
    film = Film(ftn, (8, 8))
    smp = sampler or RandomSampler(2, 0, indexed=True)
    integ = integrator or PathIntegrator(3, 1.0)
    tr, opt, st = A.ftn_tile_range(), A.ftn_render_options(), A.ftn_stats()
    tr.stride, opt.device, opt.pipeline = 1, -1, pipeline
    keep = (cam, film, smp, integ, tr, opt)
    return [C.byref(cam.desc), C.byref(film.desc), C.byref(smp.desc), C.byref(integ.desc), C.byref(tr), C.byref(opt)], st, keep


def test_refusals_come_before_the_device(ftn):
    """null arguments, the tile-serial sampler and the megakernel are refused on any machine, before the device check"""
    from fountain_amd import RandomSampler
    scene = (C.c_uint8 * 65536)()                        # stands in for a handle: the refusals never look at it
    px, mo = np.zeros((8, 8, 4), F32), np.zeros((8, 8, 4), F32)
    P, M = px.ctypes.data_as(C.c_void_p), mo.ctypes.data_as(C.c_void_p)
    args, st, keep = _args(ftn)
    assert ftn.lib.ftn_render_moments(None, *args, P, M, C.byref(st)) == A.FTN_ERR_INVALID_ARGUMENT
    assert ftn.lib.ftn_render_moments(C.byref(scene), *args, None, M, C.byref(st)) == A.FTN_ERR_INVALID_ARGUMENT
    assert ftn.lib.ftn_render_moments(C.byref(scene), *args, P, None, C.byref(st)) == A.FTN_ERR_INVALID_ARGUMENT
    assert ftn.lib.ftn_render_moments(C.byref(scene), *args[:3], None, *args[4:], P, M, C.byref(st)) == A.FTN_ERR_INVALID_ARGUMENT
    assert ftn.lib.ftn_render_moments_device(C.byref(scene), *args, P, None, None, C.byref(st)) == A.FTN_ERR_INVALID_ARGUMENT
    assert ftn.lib.ftn_render_moments_device(C.byref(scene), *args, None, M, None, C.byref(st)) == A.FTN_ERR_INVALID_ARGUMENT
    for kw in (dict(sampler=RandomSampler(2, 0)), dict(pipeline=A.FTN_PIPELINE_MEGAKERNEL)):
        args, st, keep = _args(ftn, **kw)
        assert ftn.lib.ftn_render_moments(C.byref(scene), *args, P, M, C.byref(st)) == A.FTN_ERR_UNSUPPORTED, kw
        assert ftn.lib.ftn_render_moments_device(C.byref(scene), *args, P, M, None, C.byref(st)) == A.FTN_ERR_UNSUPPORTED, kw
    assert not px.any() and not mo.any()


def test_render_without_gpu_reports_no_device(ftn):
    """No CPU fallback: with valid arguments (path, direct-lighting and Whitted integrators, AUTO and WAVEFRONT) and no device the call
    fails with FTN_ERR_NO_DEVICE"""
    if ftn.fn("device_count")() > 0:
        pytest.skip("a GPU is present")
    from fountain_amd import DirectLightingIntegrator, PathIntegrator
    scene = (C.c_uint8 * 65536)()
    px, mo = np.zeros((8, 8, 4), F32), np.zeros((8, 8, 4), F32)
    P, M = px.ctypes.data_as(C.c_void_p), mo.ctypes.data_as(C.c_void_p)
    for integ in (PathIntegrator(3, 1.0), DirectLightingIntegrator(3)):
        for pl in (A.FTN_PIPELINE_AUTO, A.FTN_PIPELINE_WAVEFRONT):
            args, st, keep = _args(ftn, integrator=integ, pipeline=pl)
            assert ftn.lib.ftn_render_moments(C.byref(scene), *args, P, M, C.byref(st)) == A.FTN_ERR_NO_DEVICE
            assert ftn.lib.ftn_render_moments_device(C.byref(scene), *args, P, M, None, C.byref(st)) == A.FTN_ERR_NO_DEVICE
    assert ftn.lib.ftn_moments_resolve_device(P, M, C.c_size_t(1), P, None) == A.FTN_ERR_NO_DEVICE


def test_oracle_backend_has_no_moments(orc):
    from fountain_amd import FountainError, moments
    with pytest.raises(FountainError) as e:
        moments.resolve(orc, np.zeros((1, 1, 4), F32), np.zeros((1, 1, 4), F32))
    assert "no oracle twin" in str(e.value)


def test_cli_refusals(tmp_path):
    from fountain_amd import render
    scene = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")
    assert render.main([scene, "-o", str(tmp_path / "a.exr"), "--variance", "--exact-stream"]) == 2
    assert render.main([scene, "-o", str(tmp_path / "a.exr"), "--variance", "--gpus", "2"]) == 2
    assert not list(tmp_path.iterdir())
    assert render.variance_path("out.exr") == "out_variance.exr"
