"""The denoiser extension of the C ABI (include/fountain_hip_denoise.h) without a GPU: the header, the ctypes mirror and the library's
exports agree; the parameter block's layout, defaults and version; every refusal, on the host twin; the GPU entry points report
FTN_ERR_NO_DEVICE where there is no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fountain_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fountain_hip_denoise.h")


def denoise_header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ftn_[a-z0-9_]+)\s*\(", src)))


def test_header_mirror_and_exports_agree(ftn):
    assert denoise_header_functions() == sorted(A.DENOISE_FUNCTIONS)
    assert not set(A.DENOISE_FUNCTIONS) & set(A.DECLARED_FUNCTIONS)
    assert not set(A.DENOISE_FUNCTIONS) & set(A.GBUFFER_FUNCTIONS)
    for name in A.DENOISE_FUNCTIONS:
        assert hasattr(ftn.lib, name), "libfountain_hip.so does not export %s" % name


def test_params_layout():
    assert C.sizeof(A.ftn_denoise_params) == 32 == A.SIZES["ftn_denoise_params"]
    offsets = {name: getattr(A.ftn_denoise_params, name).offset for name, _ in A.ftn_denoise_params._fields_}
    assert offsets == {"levels": 0, "flags": 4, "sigma_color": 8, "sigma_normal": 12, "sigma_plane": 16, "albedo_eps": 20,
                       "color_eps": 24, "reserved": 28}
    header = open(HEADER).read()
    assert int(re.search(r"#define\s+FTN_DENOISE_DEMODULATE\s+(\d+)u", header).group(1)) == A.FTN_DENOISE_DEMODULATE == 1
    assert int(re.search(r"#define\s+FTN_DENOISE_MAX_LEVELS\s+(\d+)", header).group(1)) == A.FTN_DENOISE_MAX_LEVELS == 10


def test_defaults(ftn):
    p = A.ftn_denoise_params()
    C.memset(C.byref(p), 0xA5, C.sizeof(p))
    ftn.lib.ftn_denoise_params_default(C.byref(p))
    f32 = lambda v: float(np.float32(v))
    assert (p.levels, p.flags, p.reserved) == (5, A.FTN_DENOISE_DEMODULATE, 0)
    assert (p.sigma_color, p.sigma_normal, p.sigma_plane) == (f32(2.0), f32(0.3), f32(1e-4))
    assert (p.albedo_eps, p.color_eps) == (f32(1e-3), f32(1e-4))


def test_versions(ftn):
    header = open(HEADER).read()
    assert int(re.search(r"#define\s+FTN_DENOISE_ABI_VERSION\s+(\d+)", header).group(1)) == A.FTN_DENOISE_ABI_VERSION == 1
    assert ftn.lib.ftn_denoise_abi_version() == A.FTN_DENOISE_ABI_VERSION
    assert ftn.lib.ftn_abi_version() == A.FTN_ABI_VERSION == 3              # the main ABI is unchanged by the extension
    assert ftn.lib.ftn_gbuffer_abi_version() == A.FTN_GBUFFER_ABI_VERSION == 1


def _params(ftn, **kw):
    p = A.ftn_denoise_params()
    ftn.lib.ftn_denoise_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _cpu(ftn, rgb, gb, w, h, p, out):
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return ftn.lib.ftn_denoise_cpu(ptr(rgb), ptr(gb), C.c_int32(w), C.c_int32(h), None if p is None else C.byref(p), ptr(out))


BAD_PARAMS = [
    dict(levels=11), dict(levels=-1), dict(flags=2), dict(flags=0x80000001), dict(reserved=1),
    dict(sigma_color=0.0), dict(sigma_color=-1.0), dict(sigma_color=float("nan")), dict(sigma_color=float("inf")),
    dict(sigma_normal=0.0), dict(sigma_normal=float("nan")), dict(sigma_plane=-0.1), dict(sigma_plane=float("inf")),
    dict(albedo_eps=-1e-3), dict(albedo_eps=float("nan")), dict(albedo_eps=float("inf")),
    dict(color_eps=-1e-9), dict(color_eps=float("nan")), dict(color_eps=float("inf")),
]


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=lambda d: "%s=%r" % next(iter(d.items())))
def test_refused_params(ftn, bad):
    rgb, gb = np.ones((2, 3, 3), np.float32), np.ones((2, 3, 12), np.float32)
    out = np.full((2, 3, 3), 7.0, np.float32)
    assert _cpu(ftn, rgb, gb, 3, 2, _params(ftn, **bad), out) == A.FTN_ERR_INVALID_ARGUMENT
    assert ftn.lib.ftn_last_error()
    assert (out == 7.0).all()


def test_refused_shapes_and_pointers(ftn):
    rgb, gb, out = np.ones((2, 3, 3), np.float32), np.ones((2, 3, 12), np.float32), np.zeros((2, 3, 3), np.float32)
    p = _params(ftn)
    assert _cpu(ftn, rgb, gb, 3, 2, p, out) == A.FTN_OK
    for args in ((None, gb, 3, 2, p, out), (rgb, None, 3, 2, p, out), (rgb, gb, 3, 2, None, out), (rgb, gb, 3, 2, p, None),
                 (rgb, gb, 0, 2, p, out), (rgb, gb, 3, 0, p, out), (rgb, gb, -3, 2, p, out), (rgb, gb, 3, -1, p, out),
                 (rgb, gb, 1 << 16, 1 << 15, p, out), (rgb, gb, 2 ** 31 - 1, 2, p, out)):
        assert _cpu(ftn, *args) == A.FTN_ERR_INVALID_ARGUMENT, args[2:4]
        assert ftn.lib.ftn_last_error()
    n = C.c_size_t(0)
    assert ftn.lib.ftn_denoise_workspace_size(C.c_int32(3), C.c_int32(2), C.byref(n)) == A.FTN_OK and n.value == 64 * 6
    assert ftn.lib.ftn_denoise_workspace_size(C.c_int32(4096), C.c_int32(4096), C.byref(n)) == A.FTN_OK and n.value == 64 * 4096 * 4096
    assert ftn.lib.ftn_denoise_workspace_size(C.c_int32(0), C.c_int32(2), C.byref(n)) == A.FTN_ERR_INVALID_ARGUMENT
    assert ftn.lib.ftn_denoise_workspace_size(C.c_int32(1 << 16), C.c_int32(1 << 15), C.byref(n)) == A.FTN_ERR_INVALID_ARGUMENT
    assert ftn.lib.ftn_denoise_workspace_size(C.c_int32(3), C.c_int32(2), None) == A.FTN_ERR_INVALID_ARGUMENT


def test_device_path_refusals_need_no_device(ftn):
    """The device entry point checks its arguments, the overlaps among them included, before it looks for a device: the pointers are
    only compared, never dereferenced."""
    w, h = 8, 4
    n = w * h
    p = _params(ftn)
    base = 1 << 32
    rgb, gb, out, ws = base, base + 12 * n, base + 64 * n, base + 128 * n            # disjoint ranges (12, 48, 12, 64 bytes a pixel)
    call = lambda r, g, o, wk, pp=p, ww=w, hh=h: ftn.lib.ftn_denoise_device(C.c_void_p(r), C.c_void_p(g), C.c_int32(ww), C.c_int32(hh),
                                                                           None if pp is None else C.byref(pp), C.c_void_p(o), C.c_void_p(wk), None)
    for args in ((None, gb, out, ws), (rgb, None, out, ws), (rgb, gb, None, ws), (rgb, gb, out, None)):
        assert call(*args) == A.FTN_ERR_INVALID_ARGUMENT
    assert call(rgb, gb, out, ws, pp=None) == A.FTN_ERR_INVALID_ARGUMENT
    assert call(rgb, gb, out, ws, pp=_params(ftn, levels=11)) == A.FTN_ERR_INVALID_ARGUMENT
    assert call(rgb, gb, out, ws, ww=0) == A.FTN_ERR_INVALID_ARGUMENT
    for o in (rgb, rgb + 12 * n - 4, gb + 4, ws + 64 * n - 4, rgb - 12 * n + 4):      # out_rgb overlapping an input or the workspace
        assert call(rgb, gb, o, ws) == A.FTN_ERR_INVALID_ARGUMENT, o - base
        assert b"overlap" in ftn.lib.ftn_last_error()
    for wk in (rgb + 4 * 4, gb + 48 * n - 16):                                         # the workspace overlapping an input
        assert call(rgb, gb, base + 1024 * n, wk) == A.FTN_ERR_INVALID_ARGUMENT
    assert call(rgb, gb, out, ws + 4) == A.FTN_ERR_INVALID_ARGUMENT                     # workspace not 16-byte aligned
    if ftn.fn("device_count")() == 0:                   # (with a device these calls would run on the made-up addresses)
        assert call(rgb, gb, out, ws) == A.FTN_ERR_NO_DEVICE
        assert call(rgb, gb, ws + 64 * n, ws) == A.FTN_ERR_NO_DEVICE                   # adjacent ranges do not overlap


def test_no_device(ftn):
    """No CPU fallback for the GPU entry points: with valid arguments and no device they fail with FTN_ERR_NO_DEVICE."""
    if ftn.fn("device_count")() > 0:
        pytest.skip("a GPU is present")
    rgb, gb, out = np.ones((2, 3, 3), np.float32), np.ones((2, 3, 12), np.float32), np.full((2, 3, 3), 7.0, np.float32)
    p = _params(ftn)
    assert ftn.lib.ftn_denoise(rgb.ctypes.data_as(C.c_void_p), gb.ctypes.data_as(C.c_void_p), C.c_int32(3), C.c_int32(2), C.byref(p),
                               out.ctypes.data_as(C.c_void_p), C.c_int32(-1)) == A.FTN_ERR_NO_DEVICE
    assert (out == 7.0).all()
    assert ftn.lib.ftn_denoise(None, gb.ctypes.data_as(C.c_void_p), C.c_int32(3), C.c_int32(2), C.byref(p),
                               out.ctypes.data_as(C.c_void_p), C.c_int32(-1)) == A.FTN_ERR_INVALID_ARGUMENT


def test_oracle_backend_has_no_denoiser(orc):
    from fountain_amd import FountainError, denoise
    with pytest.raises(FountainError) as e:
        denoise.denoise_cpu(orc, np.zeros((1, 1, 3), np.float32), np.zeros((1, 1, 12), np.float32))
    assert "no oracle twin" in str(e.value)


def test_python_wrappers_check_arguments(ftn):
    from fountain_amd import FountainError, denoise
    with pytest.raises(ValueError):
        denoise.denoise_cpu(ftn, np.zeros((2, 2, 3), np.float32), np.zeros((2, 3, 12), np.float32))
    with pytest.raises(TypeError):
        denoise.default_params(ftn, sigma=1.0)
    with pytest.raises(FountainError) as e:
        denoise.denoise_cpu(ftn, np.zeros((2, 2, 3), np.float32), np.zeros((2, 2, 12), np.float32), dict(levels=11))
    assert e.value.code == A.FTN_ERR_INVALID_ARGUMENT


def test_cli_refusals(tmp_path):
    from fountain_amd import render
    scene = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")
    assert render.main([scene, "-o", str(tmp_path / "a.exr"), "--denoise", "--exact-stream"]) == 2
    assert render.main([scene, "-o", str(tmp_path / "a.exr"), "--denoise", "--gpus", "2"]) == 2
    assert render.main([scene, "-o", str(tmp_path / "a.exr"), "--denoise", "--gpus", "1"]) == 2
    assert not list(tmp_path.iterdir())
    assert render.denoised_path("out.exr") == "out_denoised.exr"
