"""The temporal accumulation extension of the C ABI (include/fountain_hip_temporal.h) without a GPU: the header, the ctypes mirror and the
library's exports agree and are disjoint from the other extensions; the layouts of the parameter block and of a history pixel, the
defaults and the version; every refusal, on the host twin and on the device entry point; FTN_ERR_NO_DEVICE without a GPU; the oracle
backend's refusal; the Python wrappers' argument checks; the CLI's refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fountain_amd import _abi as A

import _temporal_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fountain_hip_temporal.h")
CORNELL = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")
W, H = 3, 2


def header_source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_mirror_and_exports_agree(ftn):
    assert sorted(set(re.findall(r"\b(ftn_[a-z0-9_]+)\s*\(", header_source()))) == sorted(A.TEMPORAL_FUNCTIONS)
    for other in (A.DECLARED_FUNCTIONS, A.GBUFFER_FUNCTIONS, A.DENOISE_FUNCTIONS, A.DENOISE_GUIDED_FUNCTIONS, A.MOMENTS_FUNCTIONS, A.ADAPTIVE_FUNCTIONS):
        assert not set(A.TEMPORAL_FUNCTIONS) & set(other)
    for name in A.TEMPORAL_FUNCTIONS:
        assert hasattr(ftn.lib, name), "libfountain_hip.so does not export %s" % name


def test_layouts():
    assert C.sizeof(A.ftn_temporal_params) == 32 == A.SIZES["ftn_temporal_params"]
    assert C.sizeof(A.ftn_temporal_pixel) == 32 == A.SIZES["ftn_temporal_pixel"]
    offsets = lambda t: {name: getattr(t, name).offset for name, _ in t._fields_}
    assert offsets(A.ftn_temporal_params) == {"flags": 0, "alpha_min": 4, "normal_tol": 8, "plane_tol": 12, "albedo_eps": 16, "albedo_tol": 20, "reserved": 24}
    assert offsets(A.ftn_temporal_pixel) == {"u": 0, "n": 12, "nu": 16}
    src = header_source()
    for t in (A.ftn_temporal_params, A.ftn_temporal_pixel):
        body = re.search(r"typedef struct %s \{(.*?)\}" % t.__name__, src, flags=re.S).group(1)
        assert re.findall(r"(\w+)(?:\[\d+\])?;", body) == [name for name, _ in t._fields_]


def test_defaults(ftn):
    p = A.ftn_temporal_params()
    C.memset(C.byref(p), 0xA5, C.sizeof(p))
    ftn.lib.ftn_temporal_params_default(C.byref(p))
    f32 = lambda v: float(np.float32(v))
    assert (p.flags, tuple(p.reserved)) == (A.FTN_DENOISE_DEMODULATE, (0, 0)) and p.flags == R.DEFAULTS["flags"]
    got = {k: getattr(p, k) for k in ("alpha_min", "normal_tol", "plane_tol", "albedo_eps", "albedo_tol")}
    assert got == {k: f32(R.DEFAULTS[k]) for k in got}
    assert got["albedo_eps"] == f32(1e-3)
    ftn.lib.ftn_temporal_params_default(None)                           # a null pointer is ignored


def test_versions(ftn):
    header = open(HEADER).read()
    assert int(re.search(r"#define\s+FTN_TEMPORAL_ABI_VERSION\s+(\d+)", header).group(1)) == A.FTN_TEMPORAL_ABI_VERSION == 1
    assert ftn.lib.ftn_temporal_abi_version() == A.FTN_TEMPORAL_ABI_VERSION
    assert ftn.lib.ftn_denoise_guided_abi_version() == A.FTN_DENOISE_GUIDED_ABI_VERSION == 1      # the other versions are unchanged
    assert ftn.lib.ftn_denoise_abi_version() == A.FTN_DENOISE_ABI_VERSION == 1
    assert ftn.lib.ftn_moments_abi_version() == A.FTN_MOMENTS_ABI_VERSION == 1
    assert ftn.lib.ftn_gbuffer_abi_version() == A.FTN_GBUFFER_ABI_VERSION == 1
    assert ftn.lib.ftn_adaptive_abi_version() == A.FTN_ADAPTIVE_ABI_VERSION == 1
    assert ftn.lib.ftn_abi_version() == A.FTN_ABI_VERSION == 3


def _params(ftn, **kw):
    p = A.ftn_temporal_params()
    ftn.lib.ftn_temporal_params_default(C.byref(p))
    for k, v in kw.items():
        if k == "reserved":
            p.reserved[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


class Args:
    """the arguments of ftn_temporal_accumulate_cpu for a 3 x 2 second frame, each replaceable"""

    def __init__(self, ftn, **kw):
        cam = R.pinhole((0, 0, -1), (W, H), 2.0)
        z = lambda k, v=0.0: np.full((H, W, k), v, np.float32)
        self.v = dict(rgb=z(3, 1.0), gb12=z(12, 1.0), var4=z(4, 0.01), cur=R.camera_desc(A, cam), film=R.film_desc(A, (W, H)), w=W, h=H,
                      prev=R.camera_desc(A, cam), prev_gb12=z(12, 1.0), prev_history=z(8, 1.0), params=_params(ftn),
                      out_history=z(8, 7.0), out_rgb=z(3, 7.0), out_var4=z(4, 7.0))
        self.v.update(kw)

    def call(self, ftn):
        v = self.v
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        ref = lambda s: None if s is None else C.byref(s)
        return ftn.lib.ftn_temporal_accumulate_cpu(ptr(v["rgb"]), ptr(v["gb12"]), ptr(v["var4"]), ref(v["cur"]), ref(v["film"]), C.c_int32(v["w"]),
                                                   C.c_int32(v["h"]), ref(v["prev"]), ptr(v["prev_gb12"]), ptr(v["prev_history"]), ref(v["params"]),
                                                   ptr(v["out_history"]), ptr(v["out_rgb"]), ptr(v["out_var4"]))

    def untouched(self):
        return all((self.v[k] == 7.0).all() for k in ("out_history", "out_rgb", "out_var4") if self.v[k] is not None)


BAD_PARAMS = [
    dict(flags=2), dict(flags=0x80000001), dict(reserved=(0, 1)), dict(reserved=(1, 5)),
    dict(alpha_min=-0.01), dict(alpha_min=1.01), dict(alpha_min=float("nan")), dict(alpha_min=float("inf")),
    dict(normal_tol=-1e-3), dict(normal_tol=float("nan")), dict(normal_tol=float("inf")),
    dict(plane_tol=-1e-3), dict(plane_tol=float("nan")), dict(plane_tol=float("inf")),
    dict(albedo_eps=-1e-3), dict(albedo_eps=float("nan")), dict(albedo_eps=float("inf")),
    dict(albedo_tol=-1e-3), dict(albedo_tol=float("nan")), dict(albedo_tol=float("inf")),
]


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=lambda d: "%s=%r" % next(iter(d.items())))
def test_refused_params(ftn, bad):
    a = Args(ftn, params=_params(ftn, **bad))
    assert a.call(ftn) == A.FTN_ERR_INVALID_ARGUMENT
    assert b"ftn_temporal_params" in ftn.lib.ftn_last_error()
    assert a.untouched()


def test_accepted_edge_params(ftn):
    """zero tolerances and epsilon, alpha_min 0 and 1 and flags 0 are accepted"""
    for p in (dict(normal_tol=0.0, plane_tol=0.0, albedo_eps=0.0, albedo_tol=0.0), dict(alpha_min=0.0), dict(alpha_min=1.0), dict(flags=0)):
        assert Args(ftn, params=_params(ftn, **p)).call(ftn) == A.FTN_OK, p


def test_refused_shapes_and_pointers(ftn):
    assert Args(ftn).call(ftn) == A.FTN_OK
    assert Args(ftn, prev=None, prev_gb12=None, prev_history=None).call(ftn) == A.FTN_OK          # the first frame
    for k in ("rgb", "gb12", "var4", "cur", "film", "params", "out_history", "out_rgb", "out_var4"):
        a = Args(ftn, **{k: None})
        assert a.call(ftn) == A.FTN_ERR_INVALID_ARGUMENT, k
        assert ftn.lib.ftn_last_error() and a.untouched()
    for nulls in (("prev",), ("prev_gb12",), ("prev_history",), ("prev", "prev_gb12"), ("prev", "prev_history"), ("prev_gb12", "prev_history")):
        a = Args(ftn, **{k: None for k in nulls})
        assert a.call(ftn) == A.FTN_ERR_INVALID_ARGUMENT, nulls
        assert b"all null" in ftn.lib.ftn_last_error() and a.untouched()
    for w, h in ((0, H), (W, 0), (-W, H), (W, -1), (1 << 16, 1 << 15), (2 ** 31 - 1, 2)):
        a = Args(ftn, w=w, h=h, film=R.film_desc(A, (w, h)) if 0 < w < 1 << 20 and h > 0 else R.film_desc(A, (W, H)))
        assert a.call(ftn) == A.FTN_ERR_INVALID_ARGUMENT, (w, h)
        assert a.untouched()
    for res in ((W + 1, H), (W, H + 1), (H, W)):                                                  # a film whose crop is not w x h
        a = Args(ftn, film=R.film_desc(A, res))
        assert a.call(ftn) == A.FTN_ERR_INVALID_ARGUMENT, res
        assert b"crop" in ftn.lib.ftn_last_error() and a.untouched()
    assert Args(ftn, film=R.film_desc(A, (W, H), origin=(5, 9), full=(64, 64))).call(ftn) == A.FTN_OK   # a crop inside a larger film


def test_device_path_refusals_need_no_device(ftn):
    """The device entry point checks its arguments, and the overlaps among them, before it looks for a device: the pointers are only
    compared, never dereferenced."""
    w, h = 8, 4
    n = w * h
    cam, film, p = R.camera_desc(A, R.pinhole((0, 0, -1), (w, h), 4.0)), R.film_desc(A, (w, h)), _params(ftn)
    base = 1 << 32
    names = ("rgb", "gb12", "var4", "prev_gb12", "prev_history", "out_history", "out_rgb", "out_var4")
    size = dict(rgb=12 * n, gb12=48 * n, var4=16 * n, prev_gb12=48 * n, prev_history=32 * n, out_history=32 * n, out_rgb=12 * n, out_var4=16 * n)
    addr, at = {}, base
    for k in names:                                                       # disjoint, adjacent ranges
        addr[k] = at
        at += size[k]

    def call(pp=p, ww=w, hh=h, cur=cam, prev=cam, fd=film, **moved):
        a = dict(addr, **moved)
        vp = lambda k: None if a[k] is None else C.c_void_p(a[k])
        ref = lambda s: None if s is None else C.byref(s)
        return ftn.lib.ftn_temporal_accumulate_device(vp("rgb"), vp("gb12"), vp("var4"), ref(cur), ref(fd), C.c_int32(ww), C.c_int32(hh), ref(prev),
                                                      vp("prev_gb12"), vp("prev_history"), ref(pp), vp("out_history"), vp("out_rgb"), vp("out_var4"), None)

    for k in ("rgb", "gb12", "var4", "out_history", "out_rgb", "out_var4"):
        assert call(**{k: None}) == A.FTN_ERR_INVALID_ARGUMENT, k
    assert call(pp=None) == A.FTN_ERR_INVALID_ARGUMENT and call(cur=None) == A.FTN_ERR_INVALID_ARGUMENT and call(fd=None) == A.FTN_ERR_INVALID_ARGUMENT
    assert call(prev=None) == A.FTN_ERR_INVALID_ARGUMENT and call(prev_gb12=None) == A.FTN_ERR_INVALID_ARGUMENT
    assert call(prev_history=None) == A.FTN_ERR_INVALID_ARGUMENT and call(prev_gb12=None, prev_history=None) == A.FTN_ERR_INVALID_ARGUMENT
    assert call(pp=_params(ftn, alpha_min=2.0)) == A.FTN_ERR_INVALID_ARGUMENT
    assert call(pp=_params(ftn, reserved=(1, 3))) == A.FTN_ERR_INVALID_ARGUMENT
    assert call(ww=0) == A.FTN_ERR_INVALID_ARGUMENT and call(ww=w + 1) == A.FTN_ERR_INVALID_ARGUMENT
    for out in ("out_history", "out_rgb", "out_var4"):
        for k in names:
            if k == out:
                continue
            for where in (addr[k], addr[k] + size[k] - 16, addr[k] - size[out] + 16):   # the output overlapping an input or another output
                assert call(**{out: where}) == A.FTN_ERR_INVALID_ARGUMENT, (out, k, where - base)
                assert b"overlap" in ftn.lib.ftn_last_error()
    far = base + (1 << 20)
    for k in ("out_history", "prev_history"):
        assert call(**{k: far + 4}) == A.FTN_ERR_INVALID_ARGUMENT                       # a history not 16-byte aligned
        assert b"misaligned" in ftn.lib.ftn_last_error()
    for k in ("rgb", "gb12", "var4", "prev_gb12", "out_rgb", "out_var4"):
        assert call(**{k: far + 2}) == A.FTN_ERR_INVALID_ARGUMENT, k                    # an image not 4-byte aligned
        assert b"misaligned" in ftn.lib.ftn_last_error()
    if ftn.fn("device_count")() == 0:                   # (with a device these calls would run on the made-up addresses)
        assert call() == A.FTN_ERR_NO_DEVICE                                            # adjacent ranges do not overlap
        assert call(prev=None, prev_gb12=None, prev_history=None) == A.FTN_ERR_NO_DEVICE


def test_no_device(ftn):
    """No CPU fallback for the GPU entry point: with valid arguments and no device it fails with FTN_ERR_NO_DEVICE."""
    if ftn.fn("device_count")() > 0:
        pytest.skip("a GPU is present")
    from fountain_amd import FountainError, temporal
    a = Args(ftn)
    v = a.v
    for prev in (None, (v["prev"], v["prev_gb12"], v["prev_history"])):
        with pytest.raises(FountainError) as e:
            temporal.temporal_accumulate(ftn, v["rgb"], v["gb12"], v["var4"], v["cur"], v["film"], prev)
        assert e.value.code == A.FTN_ERR_NO_DEVICE
    with pytest.raises(FountainError) as e:
        temporal.temporal_accumulate(ftn, v["rgb"], v["gb12"], v["var4"], v["cur"], v["film"], None, dict(alpha_min=2.0))
    assert e.value.code == A.FTN_ERR_INVALID_ARGUMENT
    with pytest.raises(FountainError) as e:
        temporal.TemporalAccumulator(ftn).push(v["rgb"], v["gb12"], v["var4"], v["cur"], v["film"])
    assert e.value.code == A.FTN_ERR_NO_DEVICE


def test_oracle_backend_has_no_temporal_accumulation(orc):
    from fountain_amd import FountainError, temporal
    z = lambda k: np.zeros((1, 1, k), np.float32)
    cam, film = R.camera_desc(A, R.pinhole((0, 0, -1), (1, 1), 1.0)), R.film_desc(A, (1, 1))
    with pytest.raises(FountainError) as e:
        temporal.temporal_accumulate_cpu(orc, z(3), z(12), z(4), cam, film)
    assert "no oracle twin" in str(e.value)
    with pytest.raises(FountainError):
        temporal.temporal_params(orc)


def test_python_wrappers_check_arguments(ftn):
    from fountain_amd import FountainError, temporal
    z = lambda *s: np.zeros(s, np.float32)
    cam, film = R.camera_desc(A, R.pinhole((0, 0, -1), (2, 2), 1.0)), R.film_desc(A, (2, 2))
    cpu = temporal.temporal_accumulate_cpu
    for rgb, gb, var in ((z(2, 2, 3), z(2, 2, 12), z(2, 3, 4)), (z(2, 2, 3), z(2, 2, 12), z(2, 2, 3)), (z(2, 2, 3), z(2, 3, 12), z(2, 2, 4)),
                         (z(2, 2, 4), z(2, 2, 12), z(2, 2, 4))):
        with pytest.raises(ValueError):
            cpu(ftn, rgb, gb, var, cam, film)
    good = (z(2, 2, 3), z(2, 2, 12), z(2, 2, 4))
    for prev in ((cam, z(2, 2, 12)), (cam, z(2, 2, 12), None), (cam, z(2, 3, 12), z(2, 2, 8)), (cam, z(2, 2, 12), z(2, 2, 7))):
        with pytest.raises(ValueError):
            cpu(ftn, *good, cam, film, prev)
    with pytest.raises(TypeError):
        cpu(ftn, *good, film, film)                                      # a film where the camera belongs
    with pytest.raises(TypeError):
        cpu(ftn, *good, cam, cam)
    with pytest.raises(TypeError):
        cpu(ftn, *good, cam, film, (film, z(2, 2, 12), z(2, 2, 8)))
    with pytest.raises(TypeError):
        temporal.temporal_params(ftn, sigma_variance=1.0)               # a field of the guided filter's block
    with pytest.raises(TypeError):
        temporal.temporal_params(ftn, reserved=1)
    with pytest.raises(TypeError):
        from fountain_amd import denoise
        cpu(ftn, *good, cam, film, None, denoise.guided_params(ftn))
    with pytest.raises(FountainError) as e:
        cpu(ftn, *good, cam, film, None, dict(alpha_min=-1.0))
    assert e.value.code == A.FTN_ERR_INVALID_ARGUMENT
    with pytest.raises(FountainError) as e:
        cpu(ftn, *good, cam, R.film_desc(A, (3, 2)))                     # a film of another size
    assert e.value.code == A.FTN_ERR_INVALID_ARGUMENT
    p = temporal.temporal_params(ftn, alpha_min=0.25, plane_tol=0.5)
    assert (p.alpha_min, p.plane_tol, p.normal_tol) == (0.25, 0.5, np.float32(R.DEFAULTS["normal_tol"]))
    hist, rgb, var = cpu(ftn, *good, cam, film)
    assert hist.shape == (2, 2, 8) and rgb.shape == (2, 2, 3) and var.shape == (2, 2, 4) and (hist[..., 3] == 1).all()
    assert temporal.frame_paths("out.exr", 3) == ("out_3.exr", "out_3_accumulated.exr", "out_3_denoised_guided.exr")


def test_cli_refusals(tmp_path):
    from fountain_amd import temporal
    out = str(tmp_path / "out" / "a.exr")
    assert temporal.main([CORNELL, CORNELL, "-o", out, "--samples", "1"]) == 2
    assert temporal.main([CORNELL, CORNELL, "-o", out, "--samples", "1", "--denoise-guided"]) == 2
    assert temporal.main([CORNELL, CORNELL, "-o", out, "--samples", "4", "--alpha-min", "1.5"]) == 2
    other = tmp_path / "other_film.pbrt"
    text = open(CORNELL).read()
    assert '"integer xresolution" [ 64 ]' in text
    other.write_text(text.replace('"integer xresolution" [ 64 ]', '"integer xresolution" [ 48 ]'))
    assert temporal.main([CORNELL, str(other), "-o", out, "--samples", "4"]) == 2               # frames whose films differ
    for extra in (["--exact-stream"], ["--gpus", "2"], ["--adaptive", "0.05"]):                 # what --denoise-guided refuses in render.py
        with pytest.raises(SystemExit) as e:
            temporal.main([CORNELL, CORNELL, "-o", out, "--samples", "4", "--denoise-guided"] + extra)
        assert e.value.code == 2
    assert not (tmp_path / "out").exists()
