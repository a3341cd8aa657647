"""The vector-blur extension of the C ABI (include/fountain_hip_vectorblur.h) without a GPU: the header, the ctypes mirror and the library's
exports agree and are disjoint from the other extensions; the layout, the versions (every older one unchanged) and the defaults; the
workspace formula; every refusal in the header's order for the host-buffer, device and twin entries (each stage is tried with every later
stage violated as well, and the message must be its own); then FTN_ERR_NO_DEVICE where there is no GPU; the two command lines' refusals,
with nothing written."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fountain_amd import _abi as A

import _vectorblur_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fountain_hip_vectorblur.h")
F32 = np.float32
INV, NODEV = A.FTN_ERR_INVALID_ARGUMENT, A.FTN_ERR_NO_DEVICE


@pytest.fixture(scope="module")
def lib(ftn):
    from fountain_amd.vectorblur import _lib
    return _lib(ftn)


def header_source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_mirror_and_exports_agree(ftn):
    import fountain_amd
    src = header_source()
    assert sorted(set(re.findall(r"\b(ftn_[a-z0-9_]+)\s*\(", src))) == sorted(A.VECTORBLUR_FUNCTIONS) == sorted(A.VECTORBLUR_PROTOTYPES)
    others = [getattr(A, name) for name in dir(A) if name.endswith("_FUNCTIONS") and name != "VECTORBLUR_FUNCTIONS"]
    assert len(others) >= 15
    for other in others:
        assert not set(A.VECTORBLUR_FUNCTIONS) & set(other)
    for name in A.VECTORBLUR_FUNCTIONS:
        assert hasattr(ftn.lib, name), "libfountain_hip.so does not export %s" % name
        assert "motion" not in name
    # the header's prototypes take as many arguments as the mirror's
    for name, (argtypes, _) in A.VECTORBLUR_PROTOTYPES.items():
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, re.S).group(1).strip()
        assert (0 if args == "void" else len(args.split(","))) == len(argtypes), name
    # nothing of the stage is declared in the main header, whose functions all need an oracle twin
    assert "vectorblur" not in open(os.path.join(ROOT, "include", "fountain_hip.h")).read()
    import fountain_amd.vectorblur as V
    assert fountain_amd.VectorBlurParams is V.VectorBlurParams and "VectorBlurParams" in fountain_amd.__all__


def test_layout_versions_and_constants(ftn, lib):
    assert C.sizeof(A.ftn_vectorblur_params) == 32 == A.SIZES["ftn_vectorblur_params"]
    assert {name: getattr(A.ftn_vectorblur_params, name).offset for name, _ in A.ftn_vectorblur_params._fields_} == {
        "taps": 0, "flags": 4, "shutter": 8, "max_radius": 12, "depth_extent": 16, "reserved": 20}
    header = open(HEADER).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct ftn_vectorblur_params \{(.*?)\} ftn_vectorblur_params;", header, re.S).group(1), flags=re.S)
    assert re.findall(r"\b(\w+)(?:\[\d+\])?;", body) == [name for name, _ in A.ftn_vectorblur_params._fields_]
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1))
    assert define("FTN_VECTORBLUR_ABI_VERSION") == A.FTN_VECTORBLUR_ABI_VERSION == 1 == lib.ftn_vectorblur_abi_version()
    assert define("FTN_VECTORBLUR_MAX_TAPS") == A.FTN_VECTORBLUR_MAX_TAPS == 64
    assert define("FTN_VECTORBLUR_MAX_RADIUS") == A.FTN_VECTORBLUR_MAX_RADIUS == 16 == R.TILE
    # the main ABI and the other extensions are unchanged
    assert ftn.lib.ftn_abi_version() == A.FTN_ABI_VERSION == 3
    for name in ("gbuffer", "idmatte", "ao", "lightpass", "motion", "denoise", "denoise_guided", "moments", "adaptive", "temporal", "filter", "display", "bloom",
                 "metrics", "subdiv"):
        assert getattr(ftn.lib, "ftn_%s_abi_version" % name)() == getattr(A, "FTN_%s_ABI_VERSION" % name.upper()), name
    assert ftn.lib.ftn_motion_abi_version() == 1 and ftn.lib.ftn_bloom_abi_version() == 1 and ftn.lib.ftn_temporal_abi_version() == 1


def test_defaults(ftn, lib):
    from fountain_amd.vectorblur import VectorBlurParams
    d = VectorBlurParams(ftn).desc
    got = {k: getattr(d, k) for k, _ in d._fields_ if k != "reserved"}
    assert got == dict(taps=16, flags=0, shutter=0.5, max_radius=16.0, depth_extent=float(F32(0.01))) and list(d.reserved) == [0, 0, 0]
    assert {k: got[k] for k in ("taps", "shutter", "max_radius")} == {k: v for k, v in R.params().items() if k != "depth_extent"}
    lib.ftn_vectorblur_params_default(None)                               # ignored
    p = VectorBlurParams(ftn, taps=7, shutter=1.0, max_radius=4.0)
    assert (p.desc.taps, p.desc.shutter, p.desc.max_radius, p.desc.flags) == (7, 1.0, 4.0, 0)
    for bad in (dict(radius=1.0), dict(reserved=1)):
        with pytest.raises(TypeError):
            VectorBlurParams(ftn, **bad)


def test_oracle_backend_has_no_vector_blur_stage(orc):
    from fountain_amd import FountainError
    from fountain_amd.vectorblur import VectorBlurParams
    with pytest.raises(FountainError) as e:
        VectorBlurParams(orc)
    assert "no oracle twin" in str(e.value)


def test_workspace_formula(ftn, lib):
    from fountain_amd.vectorblur import workspace_size
    want = {(1, 1): 16 + 32, (1, 7): 7 * 16 + 32, (16, 16): 4096 + 32, (17, 33): 16 * 17 * 33 + 32 * 2 * 3, (4096, 4096): 16 * 4096 * 4096 + 32 * 256 * 256}
    for (w, h), nbytes in want.items():
        assert workspace_size(ftn, w, h) == nbytes == R.workspace_bytes(w, h), (w, h)
    n = C.c_size_t(77)
    assert lib.ftn_vectorblur_workspace_size(8, 8, None) == INV and "null" in ftn.fn("last_error")().decode()
    assert lib.ftn_vectorblur_workspace_size(0, 8, C.byref(n)) == INV and "positive" in ftn.fn("last_error")().decode()
    assert lib.ftn_vectorblur_workspace_size(65536, 32768, C.byref(n)) == INV and "2^31" in ftn.fn("last_error")().decode()
    assert n.value == 77


# ------------------------------------------------------------------ refusals, in the header's order
# (stage, what to violate, the words its message must hold); "p." names a field of the parameters
STAGES = [("null", None, "null argument"), ("size", None, "positive"),
          ("p.taps", 65, "taps"), ("p.flags", 1, "flags bits"), ("p.reserved", 1, "reserved"),
          ("p.max_radius", float("nan"), "must be finite"), ("p.shutter", 1.5, "out of range"),
          ("null workspace", None, "null workspace"), ("overlap", None, "overlaps"), ("align", None, "misaligned")]


class Buffers:
    """host memory standing in for device memory as well: no refusal looks behind a pointer"""

    def __init__(self, w=5, h=7):
        self.w, self.h = w, h
        pad = lambda nbytes: 16 * ((nbytes + 15) // 16)
        self.n = {"rgb": pad(12 * w * h), "motion": pad(8 * w * h), "gb12": pad(48 * w * h), "out": pad(12 * w * h), "ws": R.workspace_bytes(w, h)}
        self.store = np.zeros(sum(self.n.values()) // 4 + 64, F32)        # rgb | motion | gb12 | out_rgb | workspace, each 16-byte aligned
        base = self.store.ctypes.data
        base += (-base) % 16
        self.at = {}
        for k, nbytes in self.n.items():
            self.at[k] = base
            base += nbytes
        self.rgb, self.motion, self.gb12, self.out_rgb, self.ws = (self.at[k] for k in ("rgb", "motion", "gb12", "out", "ws"))


def _violated(ftn, entry, first, stages):
    """arguments of `entry` with every stage from `first` on violated"""
    from fountain_amd.vectorblur import VectorBlurParams
    on = stages[stages.index(first):]
    is_on = lambda name: any(s[0] == name for s in on)
    b = Buffers()
    p = VectorBlurParams(ftn).desc
    for name, value, _ in on:
        if name == "p.reserved":
            p.reserved[2] = value
        elif name.startswith("p."):
            setattr(p, name[2:], value)
    w = 0 if is_on("size") else b.w
    motion = None if is_on("null") else b.motion
    out = b.motion + 16 if is_on("overlap") else (b.out_rgb + 4 if is_on("align") else b.out_rgb)
    ws = None if is_on("null workspace") else (b.ws + 4 if is_on("align") else b.ws)
    P = C.byref(p)
    return {"vectorblur": (b.rgb, motion, b.gb12, w, b.h, P, out, -1), "vectorblur_device": (b.rgb, motion, b.gb12, w, b.h, P, out, ws, None),
            "vectorblur_cpu": (b.rgb, motion, b.gb12, w, b.h, P, out), "vectorblur_velocities_cpu": (motion, b.gb12, w, b.h, P, b.ws)}[entry], b


ENTRY_STAGES = {"vectorblur": STAGES[:7], "vectorblur_device": STAGES, "vectorblur_cpu": STAGES[:7], "vectorblur_velocities_cpu": STAGES[:7]}


@pytest.mark.parametrize("entry", sorted(ENTRY_STAGES))
def test_refusals_in_order(ftn, lib, entry):
    fn = getattr(lib, "ftn_" + entry)
    stages = ENTRY_STAGES[entry]
    for first in stages:
        args, keep = _violated(ftn, entry, first, stages)
        assert fn(*args) == INV, (entry, first[0])
        assert first[2] in ftn.fn("last_error")().decode(), (entry, first[0], ftn.fn("last_error")())
        assert not keep.store.any()


def test_further_refusals(ftn, lib):
    from fountain_amd.vectorblur import VectorBlurParams
    b = Buffers()

    def P(**fields):
        d = VectorBlurParams(ftn).desc
        for k, v in fields.items():
            if k == "reserved":
                d.reserved[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return C.byref(d)
    cpu = lambda p, w=b.w, h=b.h, rgb=b.rgb, motion=b.motion, gb=b.gb12, out=b.out_rgb: lib.ftn_vectorblur_cpu(rgb, motion, gb, w, h, p, out)
    assert cpu(P()) == 0 and cpu(P(), gb=None) == 0                                        # the G-buffer is optional
    assert cpu(None) == INV and cpu(P(), out=None) == INV and cpu(P(), rgb=None) == INV and cpu(P(), motion=None) == INV
    assert cpu(P(), w=-1) == INV and cpu(P(), h=0) == INV
    assert cpu(P(), w=65536, h=32768) == INV and "2^31" in ftn.fn("last_error")().decode()
    for kw in (dict(taps=0), dict(taps=-1), dict(taps=65), dict(flags=0x80000000), dict(flags=1), dict(reserved=(0, 1)), dict(reserved=(1, 0xffffffff)),
               dict(reserved=(2, 7)), dict(shutter=float("nan")), dict(max_radius=float("inf")), dict(depth_extent=float("inf")), dict(depth_extent=float("nan")),
               dict(shutter=-0.5), dict(shutter=1.0001), dict(max_radius=0.0), dict(max_radius=-1.0), dict(max_radius=16.5), dict(depth_extent=0.0),
               dict(depth_extent=-0.01)):
        assert cpu(P(**kw)) == INV, kw
    assert cpu(P(max_radius=17.0)) == INV and "16 x 16 tiles" in ftn.fn("last_error")().decode()        # the header says why
    for kw in (dict(taps=1), dict(taps=64), dict(shutter=0.0), dict(shutter=1.0), dict(max_radius=16.0), dict(max_radius=1e-30), dict(depth_extent=1e-30),
               dict(depth_extent=1e30)):
        assert cpu(P(**kw)) == 0, kw
    # the twin refuses an output over its input
    n = 12 * b.w * b.h
    for out in (b.rgb, b.rgb + 4, b.rgb + n - 4):
        assert cpu(P(), out=out) == INV and "overlaps rgb" in ftn.fn("last_error")().decode()
    # the device path: out_rgb against each input and the workspace, the workspace against each input; each buffer's alignment
    dev = lambda rgb=b.rgb, motion=b.motion, gb=b.gb12, out=b.out_rgb, ws=b.ws, p=None: lib.ftn_vectorblur_device(rgb, motion, gb, b.w, b.h, p or P(), out, ws, None)
    for kw in (dict(out=b.rgb), dict(out=b.rgb + n - 16), dict(out=b.motion), dict(out=b.gb12 + 16), dict(out=b.ws), dict(out=b.ws + b.n["ws"] - 16),
               dict(ws=b.rgb), dict(ws=b.motion + 16), dict(ws=b.gb12 + 48 * b.w * b.h - 16)):
        assert dev(**kw) == INV and "overlaps" in ftn.fn("last_error")().decode(), kw
    for kw in (dict(rgb=b.rgb + 4), dict(motion=b.motion + 8), dict(gb=b.gb12 - 4), dict(out=b.out_rgb + 8), dict(ws=b.ws + 4)):
        assert dev(**kw) == INV and "misaligned" in ftn.fn("last_error")().decode(), kw
    assert dev(ws=None) == INV and "null workspace" in ftn.fn("last_error")().decode()


def test_entries_that_run_on_the_gpu_report_no_device(ftn, lib):
    """No CPU fallback: valid arguments and no device -> FTN_ERR_NO_DEVICE, after every refusal"""
    if ftn.fn("device_count")() > 0:
        pytest.skip("a GPU is present")
    from fountain_amd.vectorblur import VectorBlurParams
    b = Buffers()
    for kw in (dict(), dict(taps=1, shutter=0.0), dict(max_radius=2.0)):
        p = C.byref(VectorBlurParams(ftn, **kw).desc)
        for gb in (b.gb12, None):
            assert lib.ftn_vectorblur(b.rgb, b.motion, gb, b.w, b.h, p, b.out_rgb, -1) == NODEV
            assert lib.ftn_vectorblur_device(b.rgb, b.motion, gb, b.w, b.h, p, b.out_rgb, b.ws, None) == NODEV
    assert b"no CPU fallback" in ftn.fn("last_error")()
    assert not b.store.any()


def test_cli_refusals(ftn, tmp_path):
    from fountain_amd import temporal, vectorblur
    scene = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")
    out = str(tmp_path / "a.exr")
    img, mo = str(tmp_path / "in.exr"), str(tmp_path / "in_motion.exr")
    # --vector-blur belongs to --dynamic; its shutter is checked before anything is read or rendered
    assert temporal.main([scene, scene, "-o", out, "--samples", "2", "--vector-blur"]) == 2
    assert temporal.main([scene, scene, "-o", out, "--samples", "2", "--vector-blur", "0.5"]) == 2
    for bad in ("1.5", "-0.25", "nan"):
        assert temporal.main([scene, scene, "-o", out, "--samples", "2", "--dynamic", "--vector-blur", bad]) == 2, bad
        assert vectorblur.main([img, "--motion", mo, "--shutter", bad]) == 2, bad
    for bad in (["--taps", "0"], ["--taps", "65"], ["--max-radius", "0"], ["--max-radius", "16.5"], ["--max-radius", "nan"], ["--max-radius", "-1"]):
        assert vectorblur.main([img, "--motion", mo] + bad) == 2, bad
    assert vectorblur.main([img, "--motion", mo, "-o", str(tmp_path / "out.png")]) == 2
    for bad in ([img], [img, "--motion", mo, "--taps", "two"], [img, "--motion", mo, "--gpus", "2"]):     # the motion file is required; one GPU
        with pytest.raises(SystemExit):
            vectorblur.main(bad)
    with pytest.raises(SystemExit):
        temporal.main([scene, scene, "-o", out, "--dynamic", "--vector-blur", "half"])
    assert not list(tmp_path.iterdir())
