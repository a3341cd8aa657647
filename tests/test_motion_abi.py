"""The motion extension of the C ABI (include/fountain_hip_motion.h) without a GPU: the header, the ctypes mirror and the library's exports
agree and are disjoint from the other extensions; the layout and the versions, every older version unchanged; the refusals that need no
device, in the header's order, with the output buffers untouched; FTN_ERR_NO_DEVICE where there is no GPU; the oracle backend has no twin;
what `temporal --dynamic` refuses before it renders."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fountain_amd import Film, FountainError, PerspectiveCamera, RandomSampler, _abi as A

import _temporal_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fountain_hip_motion.h")
CORNELL = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")
INV, NODEV, UNSUP = A.FTN_ERR_INVALID_ARGUMENT, A.FTN_ERR_NO_DEVICE, A.FTN_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def lib(ftn):
    from fountain_amd.motion import _lib
    return _lib(ftn)


def header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ftn_[a-z0-9_]+)\s*\(", src)))


def test_header_mirror_and_exports_agree(ftn):
    assert header_functions() == sorted(A.MOTION_FUNCTIONS) == sorted(A.MOTION_PROTOTYPES)
    others = [getattr(A, name) for name in dir(A) if name.endswith("_FUNCTIONS") and name != "MOTION_FUNCTIONS"]
    assert len(others) >= 14
    for other in others:
        assert not set(A.MOTION_FUNCTIONS) & set(other)
    for name in A.MOTION_FUNCTIONS:
        assert hasattr(ftn.lib, name), "libfountain_hip.so does not export %s" % name
    for header in ("fountain_hip.h", "fountain_hip_temporal.h", "fountain_hip_gbuffer.h"):
        assert "motion" not in re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    # the header's prototypes take as many arguments as the mirror's
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, (argtypes, _) in A.MOTION_PROTOTYPES.items():
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, re.S).group(1).strip()
        assert (0 if args == "void" else len(args.split(","))) == len(argtypes), name


def test_layout_and_versions(ftn, lib):
    off = lambda s: {name: getattr(s, name).offset for name, _ in s._fields_}
    assert C.sizeof(A.ftn_motion_pixel) == 32 == A.SIZES["ftn_motion_pixel"]
    assert off(A.ftn_motion_pixel) == {"prev_position": 0, "prev_normal": 12, "hit_weight": 24, "weight": 28}
    header = open(HEADER).read()
    body = re.search(r"typedef struct ftn_motion_pixel \{(.*?)\} ftn_motion_pixel;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+)(?:\[\d+\])?;", body) == [name for name, _ in A.ftn_motion_pixel._fields_]
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1))
    assert define("FTN_MOTION_ABI_VERSION") == A.FTN_MOTION_ABI_VERSION == 1 == lib.ftn_motion_abi_version()
    # every older version is what it was
    assert ftn.lib.ftn_abi_version() == A.FTN_ABI_VERSION == 3
    for name in ("gbuffer", "idmatte", "ao", "denoise", "denoise_guided", "moments", "adaptive", "temporal", "filter", "display", "bloom", "metrics", "subdiv"):
        assert getattr(ftn.lib, "ftn_%s_abi_version" % name)() == getattr(A, "FTN_%s_ABI_VERSION" % name.upper()), name
    assert ftn.lib.ftn_temporal_abi_version() == 1 and ftn.lib.ftn_gbuffer_abi_version() == 1 and ftn.lib.ftn_ao_abi_version() == 1


def _call_args(ftn, indexed=True, pipeline=A.FTN_PIPELINE_AUTO):
    cam = PerspectiveCamera.look_at(ftn, (0, 0, 4), (0, 0, 0), (0, 1, 0), (8, 8), fov=40.0)
    film = Film(ftn, (8, 8), (0.0, 0.0, 1.0, 1.0))
    smp = RandomSampler(2, 1, indexed=indexed)
    opt = A.ftn_render_options()
    opt.pipeline, opt.device = pipeline, -1
    return [C.byref(cam.desc), C.byref(film.desc), C.byref(smp.desc), None, C.byref(opt)], (cam, film, smp, opt)


def test_pass_refusals_and_no_device(ftn, lib):
    """Null arguments first, then (where a device exists: see test_motion.py) the scenes, then the sampler and the pipeline, then
    FTN_ERR_NO_DEVICE: there is no CPU fallback.  A scene handle is not looked behind before a device is known to exist -- without one no
    scene can have been created --, so stand-ins serve here.  No refusal writes to the caller's pixels."""
    scene = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    prev = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    raw = np.full((8, 8, 8), 7.0, np.float32)
    p_raw = raw.ctypes.data_as(C.c_void_p)
    err = lambda: ftn.fn("last_error")().decode()
    have_gpu = ftn.fn("device_count")() > 0
    for entry, tail in ((lib.ftn_render_motion, (None,)), (lib.ftn_render_motion_device, (None, None))):
        args, keep = _call_args(ftn)
        serial, keep2 = _call_args(ftn, indexed=False)
        mega, keep3 = _call_args(ftn, pipeline=A.FTN_PIPELINE_MEGAKERNEL)
        assert entry(None, prev, *args, p_raw, *tail) == INV and "null argument" in err()
        assert entry(scene, None, *args, p_raw, *tail) == INV and "null argument" in err()
        for k in range(3):
            assert entry(scene, prev, *args[:k], None, *args[k + 1:], p_raw, *tail) == INV and "null argument" in err()
        assert entry(scene, prev, *args, None, *tail) == INV and "null argument" in err()
        # null arguments come before the sampler and the pipeline
        assert entry(None, prev, *serial, p_raw, *tail) == INV and entry(scene, None, *mega, p_raw, *tail) == INV
        assert entry(scene, prev, *mega, None, *tail) == INV and "null argument" in err()
        if not have_gpu:                     # (with a device the stand-ins would be looked behind)
            assert entry(scene, prev, *serial, p_raw, *tail) == UNSUP and "FTN_SAMPLER_INDEXED" in err()
            assert entry(scene, prev, *mega, p_raw, *tail) == UNSUP and "wavefront" in err()
            both, keep4 = _call_args(ftn, indexed=False, pipeline=A.FTN_PIPELINE_MEGAKERNEL)
            assert entry(scene, prev, *both, p_raw, *tail) == UNSUP and "FTN_SAMPLER_INDEXED" in err()
            odd, keep5 = _call_args(ftn, pipeline=77)
            assert entry(scene, prev, *odd, p_raw, *tail) == INV
            assert entry(scene, prev, *args, p_raw, *tail) == NODEV and "no CPU fallback" in err()
            assert entry(scene, scene, *args, p_raw, *tail) == NODEV
    assert (raw == 7.0).all()


def test_image_stage_refusals_and_no_device(ftn, lib):
    """resolve, motion vectors and the three _motion temporal entries: their refusals need no device; the host twins run anywhere"""
    have_gpu = ftn.fn("device_count")() > 0
    err = lambda: ftn.fn("last_error")().decode()
    raw = np.full((6, 8), 7.0, np.float32)
    out = np.full((6, 8), 7.0, np.float32)
    p_raw, p_out = raw.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert lib.ftn_motion_resolve(None, 1, p_out) == INV and lib.ftn_motion_resolve(p_raw, 1, None) == INV and lib.ftn_motion_resolve(None, 0, None) == 0
    assert lib.ftn_motion_resolve_device(None, 1, p_out, None) == INV and lib.ftn_motion_resolve_device(p_raw, 1, None, None) == INV
    assert (out == 7.0).all()
    if not have_gpu:
        assert lib.ftn_motion_resolve_device(p_raw, 6, p_out, None) == NODEV and (out == 7.0).all()
    assert lib.ftn_motion_resolve(p_raw, 6, p_out) == 0 and (out[:, :3] == 1.0).all() and (out[:, 7] == 7.0).all()
    # motion vectors
    w, h = 3, 2
    cam = R.camera_desc(A, R.pinhole((0, 0, -1), (w, h), 2.0))
    film = R.film_desc(A, (w, h))
    mv8, gb12 = np.ones((h, w, 8), np.float32), np.ones((h, w, 12), np.float32)
    mo = np.full((h, w, 2), 7.0, np.float32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    ref = lambda s: None if s is None else C.byref(s)
    for fn, tail in ((lib.ftn_motion_vectors_cpu, ()), (lib.ftn_motion_vectors, (-1,)), (lib.ftn_motion_vectors_device, (None,))):
        call = lambda m=mv8, g=gb12, c=cam, p=cam, f=film, ww=w, hh=h, o=mo: fn(ptr(m), ptr(g), ref(c), ref(p), ref(f), ww, hh, ptr(o), *tail)
        for kw in (dict(m=None), dict(g=None), dict(c=None), dict(p=None), dict(f=None), dict(o=None)):
            assert call(**kw) == INV and "null argument" in err(), kw
        for ww, hh in ((0, h), (w, 0), (-1, h), (1 << 16, 1 << 15)):
            assert call(ww=ww, hh=hh) == INV
        assert call(f=R.film_desc(A, (w + 1, h))) == INV and "crop" in err()
        assert (mo == 7.0).all()
        if not have_gpu and fn is not lib.ftn_motion_vectors_cpu:
            assert call() == NODEV and (mo == 7.0).all()
    assert lib.ftn_motion_vectors_cpu(ptr(mv8), ptr(gb12), ref(cam), ref(cam), ref(film), w, h, ptr(mo)) == 0 and (mo == 0.0).all()
    # the temporal entries with mv8: temporal accumulation's own refusals, the new buffer under the same rules
    from test_temporal_abi import Args, _params
    a = Args(ftn)
    v = a.v

    def cpu(mv, **kw):
        u = dict(v, **kw)
        return lib.ftn_temporal_accumulate_motion_cpu(ptr(u["rgb"]), ptr(u["gb12"]), ptr(u["var4"]), ptr(mv), ref(u["cur"]), ref(u["film"]), u["w"], u["h"],
                                                      ref(u["prev"]), ptr(u["prev_gb12"]), ptr(u["prev_history"]), ref(u["params"]), ptr(u["out_history"]),
                                                      ptr(u["out_rgb"]), ptr(u["out_var4"]))
    mv = np.ones((2, 3, 8), np.float32)
    for k in ("rgb", "gb12", "var4", "cur", "film", "params", "out_history", "out_rgb", "out_var4"):
        assert cpu(mv, **{k: None}) == INV, k
    assert cpu(mv, prev=None) == INV and "all null" in err()
    assert cpu(mv, params=_params(ftn, alpha_min=2.0)) == INV and cpu(mv, w=0) == INV
    assert a.untouched()
    assert cpu(mv) == 0 and cpu(None) == 0
    # the device entry: the new buffer is an input under the overlap rule and needs 4-byte alignment
    n, base = 8 * 4, 1 << 32
    names = ("rgb", "gb12", "var4", "mv8", "prev_gb12", "prev_history", "out_history", "out_rgb", "out_var4")
    size = dict(rgb=12 * n, gb12=48 * n, var4=16 * n, mv8=32 * n, prev_gb12=48 * n, prev_history=32 * n, out_history=32 * n, out_rgb=12 * n, out_var4=16 * n)
    addr, at = {}, base
    for k in names:
        addr[k] = at
        at += size[k]
    cam8, film8, p = R.camera_desc(A, R.pinhole((0, 0, -1), (8, 4), 4.0)), R.film_desc(A, (8, 4)), _params(ftn)

    def dev(**moved):
        x = dict(addr, **moved)
        vp = lambda k: None if x[k] is None else C.c_void_p(x[k])
        return lib.ftn_temporal_accumulate_motion_device(vp("rgb"), vp("gb12"), vp("var4"), vp("mv8"), ref(cam8), ref(film8), 8, 4, ref(cam8), vp("prev_gb12"),
                                                         vp("prev_history"), ref(p), vp("out_history"), vp("out_rgb"), vp("out_var4"), None)
    for o in ("out_history", "out_rgb", "out_var4"):
        for where in (addr["mv8"], addr["mv8"] + size["mv8"] - 16, addr["mv8"] - size[o] + 16):
            assert dev(**{o: where}) == INV and "overlap" in err(), o
    assert dev(mv8=base + (1 << 20) + 2) == INV and "misaligned" in err()
    assert dev(rgb=None) == INV and dev(out_rgb=None) == INV
    if not have_gpu:
        assert dev() == NODEV and dev(mv8=None) == NODEV
        host = lambda mv: lib.ftn_temporal_accumulate_motion(ptr(v["rgb"]), ptr(v["gb12"]), ptr(v["var4"]), ptr(mv), ref(v["cur"]), ref(v["film"]), v["w"], v["h"],
                                                             ref(v["prev"]), ptr(v["prev_gb12"]), ptr(v["prev_history"]), ref(v["params"]),
                                                             ptr(v["out_history"]), ptr(v["out_rgb"]), ptr(v["out_var4"]), -1)
        assert host(mv) == NODEV and host(None) == NODEV


def test_oracle_backend_has_no_motion_pass(orc):
    from fountain_amd import motion as M
    with pytest.raises(FountainError) as e:
        M.motion_resolve(orc, np.zeros((1, 8), np.float32))
    assert "no oracle twin" in str(e.value)


def test_python_wrappers_check_arguments(ftn):
    from fountain_amd import motion as M, temporal as T
    z = lambda *s: np.zeros(s, np.float32)
    cam, film = R.camera_desc(A, R.pinhole((0, 0, -1), (2, 2), 1.0)), R.film_desc(A, (2, 2))
    with pytest.raises(ValueError):
        M.motion_resolve(ftn, z(4, 7))
    with pytest.raises(ValueError):
        M.motion_vectors_cpu(ftn, z(2, 2, 8), z(2, 3, 12), cam, cam, film)
    with pytest.raises(TypeError):
        M.motion_vectors_cpu(ftn, z(2, 2, 8), z(2, 2, 12), cam, film, film)
    with pytest.raises(ValueError):
        M.render_motion(ftn, None, None, None, None, scene=object())          # no previous scene
    good = (z(2, 2, 3), z(2, 2, 12), z(2, 2, 4))
    with pytest.raises(ValueError):
        T.temporal_accumulate_cpu(ftn, *good, cam, film, motion=z(2, 3, 8))
    hist, rgb, var = T.temporal_accumulate_cpu(ftn, *good, cam, film, motion=z(2, 2, 8))
    assert hist.shape == (2, 2, 8) and (hist[..., 3] == 1).all()
    assert T.motion_path("a/out.exr", 2) == "a/out_2_motion.exr"


SPHERES = """Film "image" "integer xresolution" [ 16 ] "integer yresolution" [ 16 ] "string filename" [ "f.exr" ]
Sampler "random" "integer pixelsamples" [ 2 ]
LookAt 0 -4 0  0 0 0  0 0 1
Camera "perspective" "float fov" [ 40 ]
WorldBegin
LightSource "point" "point from" [0 -3 2] "rgb I" [10 10 10]
Material "matte" "rgb Kd" [.5 .5 .5]
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 1 -1  1 1 -1  1 1 1  -1 1 1]
%s
WorldEnd
"""


def test_cli_refusals_of_dynamic(tmp_path, capsys):
    """what `temporal --dynamic` refuses before it creates a scene, renders or writes: a single frame, and files whose scenes do not
    correspond -- another primitive count, another kind in the same place, a sphere of another radius"""
    from fountain_amd import temporal
    out = str(tmp_path / "out" / "a.exr")
    assert temporal.main([CORNELL, "-o", out, "--samples", "4", "--dynamic"]) == 2
    assert "two frames" in capsys.readouterr().err
    sphere = lambda r, x=0.0: 'AttributeBegin\nTranslate %g 0 0\nShape "sphere" "float radius" %g\nAttributeEnd' % (x, r)
    tri = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0  1 0 0  0 0 1]'
    files = {}
    for name, body in (("base", sphere(0.3)), ("moved", sphere(0.3, 0.2)), ("radius", sphere(0.31, 0.2)), ("count", sphere(0.3) + "\n" + tri), ("kind", tri)):
        files[name] = tmp_path / (name + ".pbrt")
        files[name].write_text(SPHERES % body)
    for other, word in (("radius", "primitive 2, a sphere"), ("count", "primitive 3 has no counterpart"), ("kind", "primitive 2 is of another kind")):
        assert temporal.main([str(files["base"]), str(files[other]), "-o", out, "--samples", "4", "--dynamic"]) == 2, other
        assert word in capsys.readouterr().err, other
        # also when the offending pair comes later in the sequence
        assert temporal.main([str(files["base"]), str(files["moved"]), str(files[other]), "-o", out, "--samples", "4", "--dynamic"]) == 2, other
        capsys.readouterr()
    assert not (tmp_path / "out").exists()
    from fountain_amd import PbrtScene
    from fountain_amd.motion import descs_differ
    assert descs_differ(PbrtScene(str(files["base"]), ftn_backend()).desc, PbrtScene(str(files["moved"]), ftn_backend()).desc) is None


def ftn_backend():
    from fountain_amd import default_backend
    return default_backend()
