"""The light-group extension of the C ABI (include/fountain_hip_lightpass.h) without a GPU: the header, the ctypes mirror and the
library's exports agree and are disjoint from the other extensions; the layout and the versions; the refusals that need no device, in
the header's order, with the output buffers untouched; FTN_ERR_NO_DEVICE where there is no GPU; the oracle backend has no twin; what
the command line refuses."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fountain_amd import Film, FountainError, PerspectiveCamera, RandomSampler, _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fountain_hip_lightpass.h")
INV, NODEV, UNSUP = A.FTN_ERR_INVALID_ARGUMENT, A.FTN_ERR_NO_DEVICE, A.FTN_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def lib(ftn):
    from fountain_amd.lightpass import _lib
    return _lib(ftn)


def header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ftn_[a-z0-9_]+)\s*\(", src)))


def test_header_mirror_and_exports_agree(ftn):
    assert header_functions() == sorted(A.LIGHTPASS_FUNCTIONS) == sorted(A.LIGHTPASS_PROTOTYPES)
    assert len(A.LIGHTPASS_FUNCTIONS) == 8
    others = [getattr(A, name) for name in dir(A) if name.endswith("_FUNCTIONS") and name != "LIGHTPASS_FUNCTIONS"]
    assert len(others) >= 14
    for other in others:
        assert not set(A.LIGHTPASS_FUNCTIONS) & set(other)
    for name in A.LIGHTPASS_FUNCTIONS:
        assert hasattr(ftn.lib, name), "libfountain_hip.so does not export %s" % name
    assert "lightpass" not in open(os.path.join(ROOT, "include", "fountain_hip.h")).read()
    assert not [f for f in A.DECLARED_FUNCTIONS if "lightpass" in f]


def test_layout_and_versions(ftn, lib):
    off = lambda s: {name: getattr(s, name).offset for name, _ in s._fields_}
    assert C.sizeof(A.ftn_lightpass_pixel) == 32 == A.SIZES["ftn_lightpass_pixel"]
    assert off(A.ftn_lightpass_pixel) == {"lit": 0, "unshadowed": 12, "hit_weight": 24, "weight": 28}
    header = open(HEADER).read()
    body = re.search(r"typedef struct ftn_lightpass_pixel \{(.*?)\} ftn_lightpass_pixel;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+)(?:\[\d+\])?;", body) == [name for name, _ in A.ftn_lightpass_pixel._fields_]
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1))
    assert define("FTN_LIGHTPASS_ABI_VERSION") == A.FTN_LIGHTPASS_ABI_VERSION == 1 == lib.ftn_lightpass_abi_version()
    assert define("FTN_LIGHTPASS_MAX_GROUPS") == A.FTN_LIGHTPASS_MAX_GROUPS == 16
    assert ftn.lib.ftn_abi_version() == A.FTN_ABI_VERSION == 3 and ftn.lib.ftn_ao_abi_version() == 1 and ftn.lib.ftn_gbuffer_abi_version() == 1


def _call_args(ftn, indexed=True, pipeline=A.FTN_PIPELINE_AUTO):
    cam = PerspectiveCamera.look_at(ftn, (0, 0, 4), (0, 0, 0), (0, 1, 0), (8, 8), fov=40.0)
    film = Film(ftn, (8, 8), (0.0, 0.0, 1.0, 1.0))
    smp = RandomSampler(2, 1, indexed=indexed)
    opt = A.ftn_render_options()
    opt.pipeline, opt.device = pipeline, -1
    return [C.byref(cam.desc), C.byref(film.desc), C.byref(smp.desc), None, C.byref(opt)], (cam, film, smp, opt)


def _u32(*v):
    a = np.array(v, np.uint32)
    return a.ctypes.data_as(C.c_void_p), a


def test_refusals_and_no_device(ftn, lib):
    """every refusal that looks at the arguments alone comes first and in the header's order -- null arguments, the two forms of the light
    set, the indices, the sampler, the pipeline --, then FTN_ERR_NO_DEVICE: there is no CPU fallback.  Only the host-side light list of the
    scene is read before a device is known to exist, so a stand-in whose list is empty serves here.  No refusal writes to the caller's
    pixels."""
    scene = C.c_void_p(C.addressof(C.create_string_buffer(1 << 16)))         # zero bytes: a scene record with no lights
    raw = np.full((8, 8, 8), 7.0, np.float32)
    p_raw = raw.ctypes.data_as(C.c_void_p)
    err = lambda: ftn.fn("last_error")().decode()
    have_gpu = ftn.fn("device_count")() > 0
    p01, keep01 = _u32(0, 1)
    p10, keep10 = _u32(1, 0)
    p00, keep00 = _u32(0, 0)
    for entry, tail in ((lib.ftn_render_lightpass, (None,)), (lib.ftn_render_lightpass_device, (None, None))):
        args, keep = _call_args(ftn)
        serial, keep2 = _call_args(ftn, indexed=False)
        mega, keep3 = _call_args(ftn, pipeline=A.FTN_PIPELINE_MEGAKERNEL)
        # (1) null arguments, before everything else
        assert entry(None, *args, None, 0, p_raw, *tail) == INV and "null argument" in err()
        for k in range(3):
            assert entry(scene, *args[:k], None, *args[k + 1:], None, 0, p_raw, *tail) == INV and "null argument" in err()
        assert entry(scene, *args, None, 0, None, *tail) == INV and "null argument" in err()
        assert entry(scene, *serial, None, 3, None, *tail) == INV and "null argument" in err()
        # (2) the two forms of the light set, before the indices, the sampler and the pipeline
        assert entry(scene, *args, None, 2, p_raw, *tail) == INV and "light set" in err()
        assert entry(scene, *args, p10, 0, p_raw, *tail) == INV and "light set" in err()
        assert entry(scene, *serial, None, 2, p_raw, *tail) == INV and "light set" in err()
        assert entry(scene, *mega, p10, 0, p_raw, *tail) == INV and "light set" in err()
        # (3) the indices: strictly increasing, and below the scene's light count (0 here), before the sampler and the pipeline
        for p in (p10, p00):
            assert entry(scene, *args, p, 2, p_raw, *tail) == INV and ("strictly increasing" in err() or "out of range" in err())
        assert entry(scene, *args, p01, 2, p_raw, *tail) == INV and "out of range" in err()
        assert entry(scene, *args, p01, 1, p_raw, *tail) == INV and "out of range" in err()
        assert entry(scene, *serial, p01, 2, p_raw, *tail) == INV and entry(scene, *mega, p10, 2, p_raw, *tail) == INV
        # (4) the sampler, then the pipeline
        assert entry(scene, *serial, None, 0, p_raw, *tail) == UNSUP and "FTN_SAMPLER_INDEXED" in err()
        assert entry(scene, *mega, None, 0, p_raw, *tail) == UNSUP and "wavefront" in err()
        both, keep4 = _call_args(ftn, indexed=False, pipeline=A.FTN_PIPELINE_MEGAKERNEL)
        assert entry(scene, *both, None, 0, p_raw, *tail) == UNSUP and "FTN_SAMPLER_INDEXED" in err()
        odd, keep5 = _call_args(ftn, pipeline=77)
        assert entry(scene, *odd, None, 0, p_raw, *tail) == INV
        # (5) no device
        if not have_gpu:
            assert entry(scene, *args, None, 0, p_raw, *tail) == NODEV and "no CPU fallback" in err()
    assert (raw == 7.0).all()
    # resolve, compose and the term twin run anywhere; the device entries need a device
    out = np.full((64, 8), 7.0, np.float32)
    p_out = out.ctypes.data_as(C.c_void_p)
    assert lib.ftn_lightpass_resolve(None, 1, p_out) == INV and lib.ftn_lightpass_resolve(p_raw, 1, None) == INV
    assert lib.ftn_lightpass_resolve(None, 0, None) == 0
    assert lib.ftn_lightpass_resolve_device(None, 1, p_out, None) == INV and lib.ftn_lightpass_resolve_device(p_raw, 1, None, None) == INV
    assert (out == 7.0).all()
    gb, res8, rgb = np.zeros((4, 12), np.float32), np.zeros((2, 4, 8), np.float32), np.full((4, 3), 7.0, np.float32)
    gains = np.ones((2, 3), np.float32)
    pg, pr, po, pk = (a.ctypes.data_as(C.c_void_p) for a in (gb, res8, rgb, gains))
    for fn, tail in ((lib.ftn_lightpass_compose, ()), (lib.ftn_lightpass_compose_device, (None,))):
        assert fn(None, pr, 2, pk, 4, po, *tail) == INV and fn(pg, None, 2, pk, 4, po, *tail) == INV and fn(pg, pr, 2, pk, 4, None, *tail) == INV
        assert fn(pg, pr, 2, None, 4, po, *tail) == INV and fn(None, None, 2, None, 0, None, *tail) == INV and "null argument" in err()
        assert fn(pg, pr, 0, pk, 4, po, *tail) == INV and "1 to 16" in err()
        assert fn(pg, pr, 17, pk, 4, po, *tail) == INV and "1 to 16" in err()
        assert fn(pg, pr, 16, pk, 1 << 27, po, *tail) == INV and "2^31" in err()
        for bad in (float("nan"), float("inf"), float("-inf")):
            g2 = gains.copy(); g2[1, 2] = bad
            assert fn(pg, pr, 2, g2.ctypes.data_as(C.c_void_p), 4, po, *tail) == INV and "finite" in err()
        assert fn(pg, pr, 2, pk, 4, pr, *tail) == INV and "overlaps" in err()                    # the output on an input
        assert fn(pg, pr, 2, pk, 4, C.c_void_p(gb.ctypes.data + 16), *tail) == INV and "overlaps" in err()
    big = np.zeros(64, np.float32)
    base = big.ctypes.data + (-big.ctypes.data) % 16
    assert lib.ftn_lightpass_compose_device(C.c_void_p(base + 4), pr, 2, pk, 1, po, None) == INV and "misaligned" in err()
    assert (rgb == 7.0).all()
    if not have_gpu:
        assert lib.ftn_lightpass_resolve_device(p_raw, 64, p_out, None) == NODEV and (out == 7.0).all()
        assert lib.ftn_lightpass_compose_device(pg, pr, 2, pk, 4, po, None) == NODEV and (rgb == 7.0).all()
    assert lib.ftn_lightpass_compose(pg, pr, 2, pk, 4, po) == 0 and not rgb.any()
    assert lib.ftn_lightpass_compose(None, None, 2, pk, 0, None) == 0
    e, rays = np.full((2, 3), 7.0, np.float32), np.full((2, 8), 7.0, np.float32)
    hit, l24 = np.zeros((2, 24), np.float32), np.zeros((2, 24), np.float32)
    ph, pl, pe, py = (a.ctypes.data_as(C.c_void_p) for a in (hit, l24, e, rays))
    for a in ((None, pl, 2, 1, pe, py), (ph, None, 2, 1, pe, py), (ph, pl, 2, 1, None, py), (ph, pl, 2, 1, pe, None)):
        assert lib.ftn_lightpass_terms(*a) == INV
    assert (e == 7.0).all() and (rays == 7.0).all() and lib.ftn_lightpass_terms(None, None, 0, 1, None, None) == 0
    assert lib.ftn_lightpass_terms(ph, pl, 2, 1, pe, py) == 0 and not e.any() and not rays.any()      # pdf 0: no term, no ray
    assert lib.ftn_lightpass_resolve(p_raw, 64, p_out) == 0 and (out[:, 7] == 1.0).all()


def test_oracle_backend_has_no_light_pass(orc):
    from fountain_amd import lightpass as LP
    with pytest.raises(FountainError) as e:
        LP.resolve(orc, np.zeros((1, 8), np.float32))
    assert "no oracle twin" in str(e.value)


def test_cli_refusals(capsys):
    """what the command line refuses before it reads the scene file, each combination in words of its own"""
    from fountain_amd import render
    seen = []
    for argv, word in ((["x.pbrt", "--light-groups", "--exact-stream"], "default sampler"), (["x.pbrt", "--light-groups", "each", "--gpus", "2"], "one GPU"),
                       (["x.pbrt", "--light-groups", "--pixel-filter", "gaussian"], "--pixel-filter does not work with --light-groups"),
                       (["x.pbrt", "--light-groups", "kind", "--adaptive", "0.1"], "--adaptive does not work with --light-groups")):
        assert render.main(argv) == 2
        msg = capsys.readouterr().err
        assert word in msg and "--light-groups" in msg, argv
        seen.append(msg)
    assert len(set(seen)) == 4
    with pytest.raises(SystemExit):
        render.main(["x.pbrt", "--light-groups", "colour"])
    capsys.readouterr()
    assert render.lightpass_paths("a/out.exr", "point") == {"light": "a/out_light_point.exr", "lightvis": "a/out_lightvis_point.exr"}
    from fountain_amd import lightpass as LP
    for argv in (["relight", "--albedo", "a.exr", "--light", "key=k.exr:1,2", "-o", "o.exr"], ["relight", "--albedo", "a.exr", "--light", "k.exr:1,2,3", "-o", "o.exr"],
                 ["relight", "--albedo", "a.exr", "--light", "key=k.exr:1,2,nan", "-o", "o.exr"],
                 ["relight", "--albedo", "a.exr", "--light", "key=k.exr:1,2,3", "--light", "key=l.exr:1,2,3", "-o", "o.exr"],
                 ["relight", "--albedo", "a.exr", "--light", "key=k.exr:1,2,3", "-o", "o.png"]):
        assert LP.main(argv) == 2, argv
        assert "error:" in capsys.readouterr().err
    assert LP._parse_light("key=shots/a:b/k.exr:1,0.5,2") == ("key", "shots/a:b/k.exr", (1.0, 0.5, 2.0))
