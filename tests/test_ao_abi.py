"""The ambient-occlusion extension of the C ABI (include/fountain_hip_ao.h) without a GPU: the header, the ctypes mirror and the
library's exports agree and are disjoint from the other extensions; the layout and the versions; the refusals that need no device, in
the header's order, with the output buffers untouched; FTN_ERR_NO_DEVICE where there is no GPU; the oracle backend has no twin."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fountain_amd import Film, FountainError, PerspectiveCamera, RandomSampler, _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fountain_hip_ao.h")
INV, NODEV, UNSUP = A.FTN_ERR_INVALID_ARGUMENT, A.FTN_ERR_NO_DEVICE, A.FTN_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def lib(ftn):
    from fountain_amd.ao import _lib
    return _lib(ftn)


def header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ftn_[a-z0-9_]+)\s*\(", src)))


def test_header_mirror_and_exports_agree(ftn):
    assert header_functions() == sorted(A.AO_FUNCTIONS) == sorted(A.AO_PROTOTYPES)
    others = [getattr(A, name) for name in dir(A) if name.endswith("_FUNCTIONS") and name != "AO_FUNCTIONS"]
    assert len(others) >= 13
    for other in others:
        assert not set(A.AO_FUNCTIONS) & set(other)
    for name in A.AO_FUNCTIONS:
        assert hasattr(ftn.lib, name), "libfountain_hip.so does not export %s" % name
    assert "ftn_ao" not in open(os.path.join(ROOT, "include", "fountain_hip.h")).read()
    assert not [f for f in A.DECLARED_FUNCTIONS if "ao" in f.split("_")]


def test_layout_and_versions(ftn, lib):
    off = lambda s: {name: getattr(s, name).offset for name, _ in s._fields_}
    assert C.sizeof(A.ftn_ao_pixel) == 32 == A.SIZES["ftn_ao_pixel"] and C.sizeof(A.ftn_ao_options) == 16 == A.SIZES["ftn_ao_options"]
    assert off(A.ftn_ao_pixel) == {"open": 0, "bent": 4, "hit_weight": 16, "weight": 20, "_pad": 24}
    assert off(A.ftn_ao_options) == {"rays": 0, "radius": 4, "_pad": 8}
    header = open(HEADER).read()
    # the header's structs, field by field, in the mirror's order
    for struct in (A.ftn_ao_pixel, A.ftn_ao_options):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct.__name__, struct.__name__), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"\b(\w+)(?:\[\d+\])?;", body) == [name for name, _ in struct._fields_]
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1))
    assert define("FTN_AO_ABI_VERSION") == A.FTN_AO_ABI_VERSION == 1 == lib.ftn_ao_abi_version()
    assert ftn.lib.ftn_abi_version() == A.FTN_ABI_VERSION == 3 and ftn.lib.ftn_gbuffer_abi_version() == 1 and ftn.lib.ftn_idmatte_abi_version() == 1


def _call_args(ftn, indexed=True, pipeline=A.FTN_PIPELINE_AUTO):
    cam = PerspectiveCamera.look_at(ftn, (0, 0, 4), (0, 0, 0), (0, 1, 0), (8, 8), fov=40.0)
    film = Film(ftn, (8, 8), (0.0, 0.0, 1.0, 1.0))
    smp = RandomSampler(2, 1, indexed=indexed)
    opt = A.ftn_render_options()
    opt.pipeline, opt.device = pipeline, -1
    return [C.byref(cam.desc), C.byref(film.desc), C.byref(smp.desc), None, C.byref(opt)], (cam, film, smp, opt)


def _ao(rays=4, radius=float("inf")):
    o = A.ftn_ao_options()
    o.rays, o.radius = rays, radius
    return o


def test_refusals_and_no_device(ftn, lib):
    """every refusal that looks at the arguments alone comes first and in the header's order -- null arguments, rays, radius, sampler,
    pipeline --, then FTN_ERR_NO_DEVICE: there is no CPU fallback.  The scene handle is not looked behind before a device is known to
    exist, so a stand-in serves here.  No refusal writes to the caller's pixels."""
    scene = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    raw = np.full((8, 8, 8), 7.0, np.float32)
    p_raw = raw.ctypes.data_as(C.c_void_p)
    err = lambda: ftn.fn("last_error")().decode()
    have_gpu = ftn.fn("device_count")() > 0
    good = _ao()
    for entry, tail in ((lib.ftn_render_ao, (None,)), (lib.ftn_render_ao_device, (None, None))):
        args, keep = _call_args(ftn)
        assert entry(None, *args, C.byref(good), p_raw, *tail) == INV and "null argument" in err()
        for k in range(3):
            assert entry(scene, *args[:k], None, *args[k + 1:], C.byref(good), p_raw, *tail) == INV
        assert entry(scene, *args, None, p_raw, *tail) == INV and "null argument" in err()
        assert entry(scene, *args, C.byref(good), None, *tail) == INV and "null argument" in err()
        # null before rays, rays before radius, both before the sampler and the pipeline
        assert entry(scene, *args, C.byref(_ao(0, -1.0)), None, *tail) == INV and "null argument" in err()
        for rays in (0, 65, 1 << 31):
            assert entry(scene, *args, C.byref(_ao(rays, -1.0)), p_raw, *tail) == INV and "1 to 64 rays" in err()
        for radius in (0.0, -0.0, -1.0, float("nan"), float("-inf")):
            assert entry(scene, *args, C.byref(_ao(64, radius)), p_raw, *tail) == INV and "radius" in err()
        serial, keep2 = _call_args(ftn, indexed=False)
        mega, keep3 = _call_args(ftn, pipeline=A.FTN_PIPELINE_MEGAKERNEL)
        assert entry(scene, *serial, C.byref(_ao(0)), p_raw, *tail) == INV and entry(scene, *mega, C.byref(_ao(4, 0.0)), p_raw, *tail) == INV
        assert entry(scene, *serial, C.byref(good), p_raw, *tail) == UNSUP and "FTN_SAMPLER_INDEXED" in err()
        assert entry(scene, *mega, C.byref(good), p_raw, *tail) == UNSUP and "wavefront" in err()
        both, keep4 = _call_args(ftn, indexed=False, pipeline=A.FTN_PIPELINE_MEGAKERNEL)
        assert entry(scene, *both, C.byref(good), p_raw, *tail) == UNSUP and "FTN_SAMPLER_INDEXED" in err()
        odd, keep5 = _call_args(ftn, pipeline=77)
        assert entry(scene, *odd, C.byref(good), p_raw, *tail) == INV
        if not have_gpu:
            for ao in (good, _ao(1, 1e-30), _ao(64, 3.0)):
                assert entry(scene, *args, C.byref(ao), p_raw, *tail) == NODEV and "no CPU fallback" in err()
    assert (raw == 7.0).all()
    # resolve and the ray twin run anywhere; the device resolve needs a device
    out = np.full((64, 6), 7.0, np.float32)
    p_out = out.ctypes.data_as(C.c_void_p)
    assert lib.ftn_ao_resolve(None, 1, 4, p_out) == INV and lib.ftn_ao_resolve(p_raw, 1, 4, None) == INV
    assert lib.ftn_ao_resolve(p_raw, 1, 0, p_out) == INV and lib.ftn_ao_resolve(p_raw, 1, 65, p_out) == INV and "1 to 64 rays" in err()
    assert lib.ftn_ao_resolve(None, 0, 4, None) == 0
    assert lib.ftn_ao_resolve_device(None, 1, 4, p_out, None) == INV and lib.ftn_ao_resolve_device(p_raw, 1, 0, p_out, None) == INV
    assert (out == 7.0).all()
    if not have_gpu:
        assert lib.ftn_ao_resolve_device(p_raw, 64, 4, p_out, None) == NODEV
        assert (out == 7.0).all()
    rays = np.full((2, 8), 7.0, np.float32)
    hit, u = np.zeros((2, 24), np.float32), np.zeros((2, 2), np.float32)
    ph, pu, pr = (a.ctypes.data_as(C.c_void_p) for a in (hit, u, rays))
    assert lib.ftn_ao_rays(None, pu, 2, 1.0, pr) == INV and lib.ftn_ao_rays(ph, None, 2, 1.0, pr) == INV and lib.ftn_ao_rays(ph, pu, 2, 1.0, None) == INV
    assert (rays == 7.0).all() and lib.ftn_ao_rays(None, None, 0, 1.0, None) == 0
    assert lib.ftn_ao_resolve(p_raw, 64, 4, p_out) == 0 and (out[:, 5] == 7.0).all()


def test_oracle_backend_has_no_ao_pass(orc):
    from fountain_amd import ao as AO
    with pytest.raises(FountainError) as e:
        AO.resolve(orc, np.zeros((1, 8), np.float32), 4)
    assert "no oracle twin" in str(e.value)


def test_cli_refusals(capsys):
    """what the command line refuses before it reads the scene file"""
    from fountain_amd import render
    for argv, word in ((["x.pbrt", "--ao-radius", "2"], "belongs to --ao"), (["x.pbrt", "--ao", "0"], "1 to 64"), (["x.pbrt", "--ao", "65"], "1 to 64"),
                       (["x.pbrt", "--ao", "--ao-radius", "0"], "above zero"), (["x.pbrt", "--ao", "--gpus", "2"], "one GPU"),
                       (["x.pbrt", "--ao", "3", "--exact-stream"], "default sampler"), (["x.pbrt", "--ao", "--pixel-filter", "gaussian"], "--ao"),
                       (["x.pbrt", "--ao", "--adaptive", "0.1"], "--ao")):
        assert render.main(argv) == 2
        assert word in capsys.readouterr().err, argv
    assert render.ao_paths("a/out.exr") == {"ao": "a/out_ao.exr", "bent": "a/out_bent.exr"}
