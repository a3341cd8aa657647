"""The variance-guided denoiser extension of the C ABI (include/fountain_hip_denoise_guided.h) without a GPU: the header, the ctypes
mirror and the library's exports agree and are disjoint from the other extensions; the parameter block's layout, defaults and version;
every refusal, on the host twin and on the device entry point; FTN_ERR_NO_DEVICE without a GPU; the oracle backend's refusal; the
Python wrappers' argument checks; the CLI's refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fountain_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fountain_hip_denoise_guided.h")
CORNELL = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")


def guided_header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ftn_[a-z0-9_]+)\s*\(", src)))


def test_header_mirror_and_exports_agree(ftn):
    assert guided_header_functions() == sorted(A.DENOISE_GUIDED_FUNCTIONS)
    for other in (A.DECLARED_FUNCTIONS, A.GBUFFER_FUNCTIONS, A.DENOISE_FUNCTIONS, A.MOMENTS_FUNCTIONS, A.ADAPTIVE_FUNCTIONS):
        assert not set(A.DENOISE_GUIDED_FUNCTIONS) & set(other)
    for name in A.DENOISE_GUIDED_FUNCTIONS:
        assert hasattr(ftn.lib, name), "libfountain_hip.so does not export %s" % name


def test_params_layout():
    assert C.sizeof(A.ftn_denoise_guided_params) == 32 == A.SIZES["ftn_denoise_guided_params"]
    offsets = {name: getattr(A.ftn_denoise_guided_params, name).offset for name, _ in A.ftn_denoise_guided_params._fields_}
    assert offsets == {"levels": 0, "flags": 4, "sigma_variance": 8, "sigma_normal": 12, "sigma_plane": 16, "albedo_eps": 20,
                       "rel_eps": 24, "reserved": 28}
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct ftn_denoise_guided_params \{(.*?)\}", src, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [name for name, _ in A.ftn_denoise_guided_params._fields_]


def test_defaults(ftn):
    import _denoise_guided_ref as GR
    p = A.ftn_denoise_guided_params()
    C.memset(C.byref(p), 0xA5, C.sizeof(p))
    ftn.lib.ftn_denoise_guided_params_default(C.byref(p))
    f32 = lambda v: float(np.float32(v))
    assert (p.levels, p.flags, p.reserved) == (5, A.FTN_DENOISE_DEMODULATE, 0)
    got = {k: getattr(p, k) for k in ("sigma_variance", "sigma_normal", "sigma_plane", "albedo_eps", "rel_eps")}
    assert got == {k: f32(GR.DEFAULTS[k]) for k in got}
    assert (p.levels, p.flags) == (GR.DEFAULTS["levels"], GR.DEFAULTS["flags"])
    ftn.lib.ftn_denoise_guided_params_default(None)                     # a null pointer is ignored


def test_versions(ftn):
    header = open(HEADER).read()
    assert int(re.search(r"#define\s+FTN_DENOISE_GUIDED_ABI_VERSION\s+(\d+)", header).group(1)) == A.FTN_DENOISE_GUIDED_ABI_VERSION == 1
    assert ftn.lib.ftn_denoise_guided_abi_version() == A.FTN_DENOISE_GUIDED_ABI_VERSION
    assert ftn.lib.ftn_denoise_abi_version() == A.FTN_DENOISE_ABI_VERSION == 1      # the other versions are unchanged
    assert ftn.lib.ftn_abi_version() == A.FTN_ABI_VERSION == 3


def _params(ftn, **kw):
    p = A.ftn_denoise_guided_params()
    ftn.lib.ftn_denoise_guided_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _cpu(ftn, rgb, gb, var, w, h, p, out):
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return ftn.lib.ftn_denoise_guided_cpu(ptr(rgb), ptr(gb), ptr(var), C.c_int32(w), C.c_int32(h), None if p is None else C.byref(p), ptr(out))


def _inputs():
    return np.ones((2, 3, 3), np.float32), np.ones((2, 3, 12), np.float32), np.full((2, 3, 4), 0.01, np.float32)


BAD_PARAMS = [
    dict(levels=11), dict(levels=-1), dict(flags=2), dict(flags=0x80000001), dict(reserved=1),
    dict(sigma_variance=0.0), dict(sigma_variance=-1.0), dict(sigma_variance=float("nan")), dict(sigma_variance=float("inf")),
    dict(sigma_normal=0.0), dict(sigma_normal=float("nan")), dict(sigma_plane=-0.1), dict(sigma_plane=float("inf")),
    dict(albedo_eps=-1e-3), dict(albedo_eps=float("nan")), dict(albedo_eps=float("inf")),
    dict(rel_eps=-1e-9), dict(rel_eps=float("nan")), dict(rel_eps=float("inf")),
]


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=lambda d: "%s=%r" % next(iter(d.items())))
def test_refused_params(ftn, bad):
    rgb, gb, var = _inputs()
    out = np.full((2, 3, 3), 7.0, np.float32)
    assert _cpu(ftn, rgb, gb, var, 3, 2, _params(ftn, **bad), out) == A.FTN_ERR_INVALID_ARGUMENT
    assert b"ftn_denoise_guided_params" in ftn.lib.ftn_last_error()
    assert (out == 7.0).all()


def test_accepted_edge_params(ftn):
    """zero epsilons, levels 0 and 10 and flags 0 are accepted"""
    rgb, gb, var = _inputs()
    for p in (dict(albedo_eps=0.0, rel_eps=0.0), dict(levels=0), dict(levels=10), dict(flags=0)):
        out = np.zeros((2, 3, 3), np.float32)
        assert _cpu(ftn, rgb, gb, var, 3, 2, _params(ftn, **p), out) == A.FTN_OK, p


def test_refused_shapes_and_pointers(ftn):
    rgb, gb, var = _inputs()
    out = np.zeros((2, 3, 3), np.float32)
    p = _params(ftn)
    assert _cpu(ftn, rgb, gb, var, 3, 2, p, out) == A.FTN_OK
    for args in ((None, gb, var, 3, 2, p, out), (rgb, None, var, 3, 2, p, out), (rgb, gb, None, 3, 2, p, out), (rgb, gb, var, 3, 2, None, out),
                 (rgb, gb, var, 3, 2, p, None), (rgb, gb, var, 0, 2, p, out), (rgb, gb, var, 3, 0, p, out), (rgb, gb, var, -3, 2, p, out),
                 (rgb, gb, var, 3, -1, p, out), (rgb, gb, var, 1 << 16, 1 << 15, p, out), (rgb, gb, var, 2 ** 31 - 1, 2, p, out)):
        assert _cpu(ftn, *args) == A.FTN_ERR_INVALID_ARGUMENT, args[3:5]
        assert ftn.lib.ftn_last_error()
    n = C.c_size_t(0)
    ws = ftn.lib.ftn_denoise_guided_workspace_size
    assert ws(C.c_int32(3), C.c_int32(2), C.byref(n)) == A.FTN_OK and n.value == 64 * 6
    assert ws(C.c_int32(4096), C.c_int32(4096), C.byref(n)) == A.FTN_OK and n.value == 64 * 4096 * 4096
    assert ws(C.c_int32(0), C.c_int32(2), C.byref(n)) == A.FTN_ERR_INVALID_ARGUMENT
    assert ws(C.c_int32(1 << 16), C.c_int32(1 << 15), C.byref(n)) == A.FTN_ERR_INVALID_ARGUMENT
    assert ws(C.c_int32(3), C.c_int32(2), None) == A.FTN_ERR_INVALID_ARGUMENT


def test_device_path_refusals_need_no_device(ftn):
    """The device entry point checks its arguments, the overlaps among them and with var4 included, before it looks for a device: the
    pointers are only compared, never dereferenced."""
    w, h = 8, 4
    n = w * h
    p = _params(ftn)
    base = 1 << 32
    rgb, gb, var, out, ws = base, base + 12 * n, base + 64 * n, base + 96 * n, base + 128 * n    # disjoint (12, 48, 16, 12, 64 B a pixel)
    call = lambda r, g, v, o, wk, pp=p, ww=w, hh=h: ftn.lib.ftn_denoise_guided_device(
        C.c_void_p(r), C.c_void_p(g), C.c_void_p(v), C.c_int32(ww), C.c_int32(hh), None if pp is None else C.byref(pp), C.c_void_p(o),
        C.c_void_p(wk), None)
    for args in ((None, gb, var, out, ws), (rgb, None, var, out, ws), (rgb, gb, None, out, ws), (rgb, gb, var, None, ws), (rgb, gb, var, out, None)):
        assert call(*args) == A.FTN_ERR_INVALID_ARGUMENT
    assert call(rgb, gb, var, out, ws, pp=None) == A.FTN_ERR_INVALID_ARGUMENT
    assert call(rgb, gb, var, out, ws, pp=_params(ftn, levels=11)) == A.FTN_ERR_INVALID_ARGUMENT
    assert call(rgb, gb, var, out, ws, pp=_params(ftn, reserved=3)) == A.FTN_ERR_INVALID_ARGUMENT
    assert call(rgb, gb, var, out, ws, ww=0) == A.FTN_ERR_INVALID_ARGUMENT
    for o in (rgb, rgb + 12 * n - 4, gb + 4, var, var + 16 * n - 4, ws + 64 * n - 4, rgb - 12 * n + 4):   # out_rgb overlapping an input or the workspace
        assert call(rgb, gb, var, o, ws) == A.FTN_ERR_INVALID_ARGUMENT, o - base
        assert b"overlap" in ftn.lib.ftn_last_error()
    for wk in (rgb + 4 * 4, gb + 48 * n - 16, var, var + 16 * n - 16):                           # the workspace overlapping an input
        assert call(rgb, gb, var, base + 1024 * n, wk) == A.FTN_ERR_INVALID_ARGUMENT
        assert b"overlap" in ftn.lib.ftn_last_error()
    assert call(rgb, gb, var, out, ws + 4) == A.FTN_ERR_INVALID_ARGUMENT                          # workspace not 16-byte aligned
    assert call(rgb, gb, var + 2, out, ws) == A.FTN_ERR_INVALID_ARGUMENT                          # var4 not 4-byte aligned
    assert b"misaligned" in ftn.lib.ftn_last_error()
    if ftn.fn("device_count")() == 0:                   # (with a device these calls would run on the made-up addresses)
        assert call(rgb, gb, var, out, ws) == A.FTN_ERR_NO_DEVICE
        assert call(rgb, gb, var, ws + 64 * n, ws) == A.FTN_ERR_NO_DEVICE                        # adjacent ranges do not overlap


def test_no_device(ftn):
    """No CPU fallback for the GPU entry points: with valid arguments and no device they fail with FTN_ERR_NO_DEVICE."""
    if ftn.fn("device_count")() > 0:
        pytest.skip("a GPU is present")
    rgb, gb, var = _inputs()
    out = np.full((2, 3, 3), 7.0, np.float32)
    p = _params(ftn)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    call = lambda r, g, v: ftn.lib.ftn_denoise_guided(ptr(r), ptr(g), ptr(v), C.c_int32(3), C.c_int32(2), C.byref(p), ptr(out), C.c_int32(-1))
    assert call(rgb, gb, var) == A.FTN_ERR_NO_DEVICE
    assert (out == 7.0).all()
    assert call(rgb, gb, None) == A.FTN_ERR_INVALID_ARGUMENT


def test_oracle_backend_has_no_guided_denoiser(orc):
    from fountain_amd import FountainError, denoise
    with pytest.raises(FountainError) as e:
        denoise.denoise_guided_cpu(orc, np.zeros((1, 1, 3), np.float32), np.zeros((1, 1, 12), np.float32), np.zeros((1, 1, 4), np.float32))
    assert "no oracle twin" in str(e.value)
    with pytest.raises(FountainError):
        denoise.guided_params(orc)


def test_python_wrappers_check_arguments(ftn):
    from fountain_amd import FountainError, denoise
    z = lambda *s: np.zeros(s, np.float32)
    with pytest.raises(ValueError):
        denoise.denoise_guided_cpu(ftn, z(2, 2, 3), z(2, 2, 12), z(2, 3, 4))
    with pytest.raises(ValueError):
        denoise.denoise_guided_cpu(ftn, z(2, 2, 3), z(2, 2, 12), z(2, 2, 3))
    with pytest.raises(ValueError):
        denoise.denoise_guided_cpu(ftn, z(2, 2, 3), z(2, 3, 12), z(2, 2, 4))
    with pytest.raises(TypeError):
        denoise.guided_params(ftn, sigma_color=1.0)                    # a field of ftn_denoise_params, not of the guided block
    with pytest.raises(TypeError):
        denoise.denoise_guided_cpu(ftn, z(2, 2, 3), z(2, 2, 12), z(2, 2, 4), denoise.default_params(ftn))
    with pytest.raises(FountainError) as e:
        denoise.denoise_guided_cpu(ftn, z(2, 2, 3), z(2, 2, 12), z(2, 2, 4), dict(levels=11))
    assert e.value.code == A.FTN_ERR_INVALID_ARGUMENT
    p = denoise.guided_params(ftn, levels=2, sigma_variance=3.0)
    assert (p.levels, p.sigma_variance, p.sigma_normal) == (2, 3.0, np.float32(0.3))
    assert denoise.guided_workspace_bytes(ftn, 5, 7) == 64 * 35


def test_cli_refusals(tmp_path):
    from fountain_amd import render
    out = str(tmp_path / "a.exr")
    for extra in (["--exact-stream"], ["--gpus", "2"], ["--gpus", "1"], ["--adaptive", "0.05"], ["--adaptive", "0.05", "--denoise"],
                  ["--samples", "1"], ["--samples", "1", "--denoise"], ["--samples", "1", "--variance"]):
        assert render.main([CORNELL, "-o", out, "--denoise-guided"] + extra) == 2, extra
    assert render.main([CORNELL, "-o", out, "--adaptive", "0.05", "--denoise"]) == 2          # still refused on its own
    assert not list(tmp_path.iterdir())
    assert render.denoised_guided_path("out.exr") == "out_denoised_guided.exr"
