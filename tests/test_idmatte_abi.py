"""The ID-matte extension of the C ABI (include/fountain_hip_idmatte.h) without a GPU: the header, the ctypes mirror and the library's
exports agree and are disjoint from the other extensions; the layout and the versions; the refusals that need no device, in the header's
order; FTN_ERR_NO_DEVICE where there is no GPU; the oracle backend has no twin."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fountain_amd import Film, FountainError, PerspectiveCamera, RandomSampler, _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fountain_hip_idmatte.h")
INV, NODEV, UNSUP = A.FTN_ERR_INVALID_ARGUMENT, A.FTN_ERR_NO_DEVICE, A.FTN_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def lib(ftn):
    from fountain_amd.idmatte import _lib
    return _lib(ftn)


def header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ftn_[a-z0-9_]+)\s*\(", src)))


def test_header_mirror_and_exports_agree(ftn):
    assert header_functions() == sorted(A.IDMATTE_FUNCTIONS) == sorted(A.IDMATTE_PROTOTYPES)
    others = [getattr(A, name) for name in dir(A) if name.endswith("_FUNCTIONS") and name != "IDMATTE_FUNCTIONS"]
    assert len(others) >= 12
    for other in others:
        assert not set(A.IDMATTE_FUNCTIONS) & set(other)
    for name in A.IDMATTE_FUNCTIONS:
        assert hasattr(ftn.lib, name), "libfountain_hip.so does not export %s" % name
    assert "idmatte" not in open(os.path.join(ROOT, "include", "fountain_hip.h")).read()


def test_layout_and_versions(ftn, lib):
    offsets = {name: getattr(A.ftn_idmatte_pixel, name).offset for name, _ in A.ftn_idmatte_pixel._fields_}
    assert C.sizeof(A.ftn_idmatte_pixel) == 80 == A.SIZES["ftn_idmatte_pixel"]
    assert offsets == {"id": 0, "weight": 32, "overflow": 64, "miss": 68, "total": 72, "n_used": 76}
    header = open(HEADER).read()
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1))
    assert define("FTN_IDMATTE_ABI_VERSION") == A.FTN_IDMATTE_ABI_VERSION == 1 == lib.ftn_idmatte_abi_version()
    assert define("FTN_IDMATTE_SLOTS") == A.FTN_IDMATTE_SLOTS == 8 and define("FTN_IDMATTE_RESOLVED_WORDS") == A.FTN_IDMATTE_RESOLVED_WORDS == 20
    assert (define("FTN_IDMATTE_SELECT_OVERFLOW"), define("FTN_IDMATTE_SELECT_MISS")) == (A.FTN_IDMATTE_SELECT_OVERFLOW, A.FTN_IDMATTE_SELECT_MISS) == (1, 2)
    assert ftn.lib.ftn_abi_version() == A.FTN_ABI_VERSION == 3 and ftn.lib.ftn_gbuffer_abi_version() == 1


def _call_args(ftn, indexed=True, radius=(0.5, 0.5), pipeline=A.FTN_PIPELINE_AUTO, first=0, count=0):
    cam = PerspectiveCamera.look_at(ftn, (0, 0, 4), (0, 0, 0), (0, 1, 0), (8, 8), fov=40.0)
    film = Film(ftn, (8, 8), (0.0, 0.0, 1.0, 1.0))
    film.desc.filter_radius[0], film.desc.filter_radius[1] = radius
    smp = RandomSampler(2, 1, indexed=indexed, first_sample=first, sample_count=count)
    opt = A.ftn_render_options()
    opt.pipeline, opt.device = pipeline, -1
    return [C.byref(cam.desc), C.byref(film.desc), C.byref(smp.desc), None, C.byref(opt)], (cam, film, smp, opt)


def test_refusals_and_no_device(ftn, lib):
    """every refusal that looks at the arguments alone comes first, then FTN_ERR_NO_DEVICE: there is no CPU fallback.  The scene handle is
    not looked behind before a device is known to exist, so a stand-in serves here."""
    scene = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    ids = np.zeros(4, np.uint32)
    raw = np.zeros((8, 8, 20), np.uint32)
    p_ids, p_raw = ids.ctypes.data_as(C.c_void_p), raw.ctypes.data_as(C.c_void_p)
    have_gpu = ftn.fn("device_count")() > 0
    for entry, tail in ((lib.ftn_render_idmatte, (None,)), (lib.ftn_render_idmatte_device, (None, None))):
        args, keep = _call_args(ftn)
        assert entry(None, *args, p_ids, 4, p_raw, *tail) == INV and "null argument" in ftn.fn("last_error")().decode()
        for k in range(3):
            assert entry(scene, *args[:k], None, *args[k + 1:], p_ids, 4, p_raw, *tail) == INV
        assert entry(scene, *args, None, 4, p_raw, *tail) == INV and entry(scene, *args, p_ids, 4, None, *tail) == INV
        args, keep = _call_args(ftn, indexed=False)
        assert entry(scene, *args, p_ids, 4, p_raw, *tail) == UNSUP and "FTN_SAMPLER_INDEXED" in ftn.fn("last_error")().decode()
        args, keep = _call_args(ftn, pipeline=A.FTN_PIPELINE_MEGAKERNEL)
        assert entry(scene, *args, p_ids, 4, p_raw, *tail) == UNSUP and "wavefront" in ftn.fn("last_error")().decode()
        args, keep = _call_args(ftn, pipeline=77)
        assert entry(scene, *args, p_ids, 4, p_raw, *tail) == INV
        for radius in ((1.5, 0.5), (0.5, 1.0000001), (float("nan"), 0.5)):
            args, keep = _call_args(ftn, radius=radius)
            assert entry(scene, *args, p_ids, 4, p_raw, *tail) == UNSUP and "3 x 3" in ftn.fn("last_error")().decode()
        args, keep = _call_args(ftn, first=1, count=2)
        assert entry(scene, *args, p_ids, 4, p_raw, *tail) == INV and "sample range" in ftn.fn("last_error")().decode()
        if not have_gpu:
            for radius in ((0.5, 0.5), (1.0, 1.0)):
                args, keep = _call_args(ftn, radius=radius)
                assert entry(scene, *args, p_ids, 4, p_raw, *tail) == NODEV and "no CPU fallback" in ftn.fn("last_error")().decode()
    assert not raw.any()
    # resolve and select: the host twins run anywhere, the device entries need a device
    out = np.zeros((8, 8, 20), np.uint32)
    mask = np.zeros((8, 8), np.float32)
    p_out, p_mask = out.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p)
    assert lib.ftn_idmatte_resolve(None, 1, p_out) == INV and lib.ftn_idmatte_resolve(p_raw, 1, None) == INV and lib.ftn_idmatte_resolve(None, 0, None) == 0
    assert lib.ftn_idmatte_select(None, 1, p_ids, 1, 0, p_mask) == INV and lib.ftn_idmatte_select(p_out, 1, None, 1, 0, p_mask) == INV
    assert lib.ftn_idmatte_select(p_out, 1, p_ids, 1, 0, None) == INV
    assert lib.ftn_idmatte_select(p_out, 1, p_ids, 1, 4, p_mask) == INV and "flag" in ftn.fn("last_error")().decode()
    assert lib.ftn_idmatte_select(p_out, 64, None, 0, 3, p_mask) == 0 and lib.ftn_idmatte_select(None, 0, None, 0, 0, None) == 0
    assert lib.ftn_idmatte_resolve_device(None, 1, p_out, None) == INV and lib.ftn_idmatte_select_device(p_out, 1, p_ids, 1, 8, p_mask, None) == INV
    if not have_gpu:
        assert lib.ftn_idmatte_resolve_device(p_raw, 64, p_out, None) == NODEV
        assert lib.ftn_idmatte_select_device(p_out, 64, p_ids, 4, 3, p_mask, None) == NODEV
        assert not out.any() and not mask.any()


def test_oracle_backend_has_no_idmatte_pass(orc):
    from fountain_amd import idmatte as I
    with pytest.raises(FountainError) as e:
        I.resolve(orc, np.zeros((1, 20), np.uint32))
    assert "no oracle twin" in str(e.value)
