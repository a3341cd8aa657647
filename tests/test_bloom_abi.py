"""The bloom extension of the C ABI (include/fountain_hip_bloom.h) without a GPU: the header, the ctypes mirror and the library's exports
agree; the layout, the version and the defaults; the workspace formula; every refusal in the header's order for the host-buffer,
device and twin entries (each stage is tried with every later stage violated as well, and the message must be its own); then
FTN_ERR_NO_DEVICE where there is no GPU; the three command lines' refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fountain_amd import _abi as A

import _bloom_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fountain_hip_bloom.h")
F32 = np.float32
INV, NODEV = A.FTN_ERR_INVALID_ARGUMENT, A.FTN_ERR_NO_DEVICE


@pytest.fixture(scope="module")
def lib(ftn):
    from fountain_amd.bloom import _lib
    return _lib(ftn)


def header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ftn_[a-z0-9_]+)\s*\(", src)))


def test_header_mirror_and_exports_agree(ftn):
    import fountain_amd
    assert header_functions() == sorted(A.BLOOM_FUNCTIONS) == sorted(A.BLOOM_PROTOTYPES)
    for other in (A.DECLARED_FUNCTIONS, A.GBUFFER_FUNCTIONS, A.DENOISE_FUNCTIONS, A.DENOISE_GUIDED_FUNCTIONS, A.MOMENTS_FUNCTIONS, A.ADAPTIVE_FUNCTIONS,
                  A.TEMPORAL_FUNCTIONS, A.FILTER_FUNCTIONS, A.DISPLAY_FUNCTIONS):
        assert not set(A.BLOOM_FUNCTIONS) & set(other)
    for name in A.BLOOM_FUNCTIONS:
        assert hasattr(ftn.lib, name), "libfountain_hip.so does not export %s" % name
    # nothing of the bloom stage is declared in the main header, whose functions all need an oracle twin
    assert "ftn_bloom" not in open(os.path.join(ROOT, "include", "fountain_hip.h")).read()
    import fountain_amd.bloom as B
    assert fountain_amd.BloomParams is B.BloomParams and "BloomParams" in fountain_amd.__all__


def test_layout_versions_and_constants(ftn, lib):
    assert C.sizeof(A.ftn_bloom_params) == 32 == A.SIZES["ftn_bloom_params"]
    assert {name: getattr(A.ftn_bloom_params, name).offset for name, _ in A.ftn_bloom_params._fields_} == {
        "levels": 0, "flags": 4, "strength": 8, "scatter": 12, "threshold": 16, "knee": 20, "clamp_max": 24, "reserved": 28}
    header = open(HEADER).read()
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1))
    assert define("FTN_BLOOM_ABI_VERSION") == A.FTN_BLOOM_ABI_VERSION == 1 == lib.ftn_bloom_abi_version()
    assert define("FTN_BLOOM_KARIS") == A.FTN_BLOOM_KARIS == 1 and define("FTN_BLOOM_MAX_LEVELS") == A.FTN_BLOOM_MAX_LEVELS == 12
    # the main ABI and the other extensions are unchanged
    assert ftn.lib.ftn_abi_version() == A.FTN_ABI_VERSION == 3
    assert ftn.lib.ftn_display_abi_version() == 1 and ftn.lib.ftn_filter_abi_version() == 1 and ftn.lib.ftn_temporal_abi_version() == 1
    assert ftn.lib.ftn_denoise_abi_version() == 1


def test_defaults(ftn, lib):
    from fountain_amd.bloom import BloomParams
    d = BloomParams(ftn).desc
    got = {k: getattr(d, k) for k, _ in d._fields_}
    assert got == dict(levels=6, flags=0, strength=float(F32(0.04)), scatter=float(F32(0.7)), threshold=0.0, knee=0.5, clamp_max=65504.0, reserved=0)
    assert {k: got[k] for k in ("levels", "strength", "scatter", "threshold", "knee", "clamp_max")} == {k: v for k, v in R.params().items() if k != "karis"}
    lib.ftn_bloom_params_default(None)                                    # ignored
    p = BloomParams(ftn, karis=True, levels=3, threshold=1.5)
    assert (p.desc.flags, p.desc.levels, p.desc.threshold) == (1, 3, 1.5)
    assert BloomParams(ftn, karis=False).desc.flags == 0
    with pytest.raises(TypeError):
        BloomParams(ftn, radius=1.0)


def test_oracle_backend_has_no_bloom_stage(orc):
    from fountain_amd import FountainError
    from fountain_amd.bloom import BloomParams
    with pytest.raises(FountainError) as e:
        BloomParams(orc)
    assert "no oracle twin" in str(e.value)


def test_workspace_formula(ftn, lib):
    from fountain_amd.bloom import workspace_size
    for w, h in ((1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (17, 31), (64, 64), (255, 257), (4096, 4096), (5000, 3)):
        for levels in range(0, 13):
            assert workspace_size(ftn, w, h, levels) == R.workspace_bytes(w, h, levels), (w, h, levels)
    assert workspace_size(ftn, 1, 1) == 0 and workspace_size(ftn, 64, 64, 0) == 0
    assert workspace_size(ftn, 3, 5, 1) == 16 * ((12 * 2 * 3 + 15) // 16) == 80
    assert workspace_size(ftn, 64, 64) == workspace_size(ftn, 64, 64, 6) == workspace_size(ftn, 64, 64, 12)     # 64 halves six times
    assert workspace_size(ftn, 4096, 4096, 1) == 12 * 2048 * 2048
    n = C.c_size_t(77)
    assert lib.ftn_bloom_workspace_size(8, 8, 6, None) == INV and "null" in ftn.fn("last_error")().decode()
    assert lib.ftn_bloom_workspace_size(0, 8, 13, C.byref(n)) == INV and "positive" in ftn.fn("last_error")().decode()
    assert lib.ftn_bloom_workspace_size(65536, 32768, 13, C.byref(n)) == INV and "2^31" in ftn.fn("last_error")().decode()
    assert lib.ftn_bloom_workspace_size(8, 8, 13, C.byref(n)) == INV and "levels" in ftn.fn("last_error")().decode()
    assert lib.ftn_bloom_workspace_size(8, 8, -1, C.byref(n)) == INV and n.value == 77


# ------------------------------------------------------------------ refusals, in the header's order
# (stage, what to violate, the words its message must hold); "p." names a field of the parameters
STAGES = [("null", None, "null argument"), ("size", None, "positive"),
          ("p.levels", 13, "levels"), ("p.flags", 2, "flags bits"), ("p.reserved", 1, "reserved"),
          ("p.knee", float("nan"), "must be finite"), ("p.strength", 1.5, "out of range"),
          ("null workspace", None, "null workspace"), ("overlap", None, "overlaps"), ("align", None, "misaligned")]


class Buffers:
    """host memory standing in for device memory as well: no refusal looks behind a pointer"""

    def __init__(self, w=5, h=7, levels=6):
        self.w, self.h = w, h
        n = 16 * ((12 * w * h + 15) // 16)
        self.ws_bytes = R.workspace_bytes(w, h, levels)
        self.store = np.zeros((2 * n + self.ws_bytes) // 4 + 64, F32)     # rgb | out_rgb | workspace, each 16-byte aligned
        base = self.store.ctypes.data
        base += (-base) % 16
        self.rgb, self.out_rgb, self.ws = base, base + n, base + 2 * n


def _violated(ftn, entry, first, stages):
    """arguments of `entry` with every stage from `first` on violated"""
    from fountain_amd.bloom import BloomParams
    on = stages[stages.index(first):]
    is_on = lambda name: any(s[0] == name for s in on)
    b = Buffers()
    p = BloomParams(ftn).desc
    for name, value, _ in on:
        if name.startswith("p."):
            setattr(p, name[2:], value)
    w = 0 if is_on("size") else b.w
    rgb = None if is_on("null") else b.rgb
    out = b.rgb + 16 if is_on("overlap") else (b.out_rgb + 4 if is_on("align") else b.out_rgb)
    ws = None if is_on("null workspace") else (b.ws + 4 if is_on("align") else b.ws)
    P = C.byref(p)
    return {"bloom": (rgb, w, b.h, P, out, -1), "bloom_device": (rgb, w, b.h, P, out, ws, None), "bloom_cpu": (rgb, w, b.h, P, out)}[entry], b


ENTRY_STAGES = {"bloom": STAGES[:7], "bloom_device": STAGES, "bloom_cpu": STAGES[:7]}


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
    from fountain_amd.bloom import BloomParams
    b = Buffers()

    def P(**fields):
        d = BloomParams(ftn).desc
        for k, v in fields.items():
            setattr(d, k, v)
        return C.byref(d)
    cpu = lambda p, w=b.w, h=b.h, rgb=b.rgb, out=b.out_rgb: lib.ftn_bloom_cpu(rgb, w, h, p, out)
    assert cpu(P()) == 0
    assert cpu(None) == INV and cpu(P(), out=None) == INV and cpu(P(), rgb=None) == INV
    assert cpu(P(), w=-1) == INV and cpu(P(), h=0) == INV
    assert cpu(P(), w=65536, h=32768) == INV and "2^31" in ftn.fn("last_error")().decode()
    for kw in (dict(levels=-1), dict(levels=13), dict(flags=0x80000000), dict(flags=3), dict(reserved=0xffffffff),
               dict(strength=float("nan")), dict(scatter=float("inf")), dict(threshold=float("inf")), dict(knee=float("-inf")), dict(clamp_max=float("nan")),
               dict(strength=-0.5), dict(strength=1.0001), dict(scatter=-1.0), dict(scatter=2.0), dict(threshold=-1.0), dict(knee=-0.1), dict(knee=1.5),
               dict(clamp_max=0.0), dict(clamp_max=-1.0), dict(clamp_max=2e30)):
        assert cpu(P(**kw)) == INV, kw
    for kw in (dict(levels=0), dict(levels=12), dict(strength=0.0), dict(strength=1.0), dict(scatter=0.0), dict(scatter=1.0), dict(threshold=1e30),
               dict(knee=0.0), dict(knee=1.0), dict(clamp_max=1e30), dict(clamp_max=1e-30), dict(flags=A.FTN_BLOOM_KARIS)):
        assert cpu(P(**kw)) == 0, kw
    # the device path: out_rgb against the input and the workspace, the workspace against the input; each buffer's alignment
    dev = lambda rgb=b.rgb, out=b.out_rgb, ws=b.ws, p=None: lib.ftn_bloom_device(rgb, b.w, b.h, p or P(), out, ws, None)
    n = 12 * b.w * b.h
    for kw in (dict(out=b.rgb), dict(out=b.rgb + n - 16), dict(out=b.ws), dict(out=b.ws + b.ws_bytes - 16), dict(ws=b.rgb), dict(ws=b.rgb + n - 16)):
        assert dev(**kw) == INV and "overlaps" in ftn.fn("last_error")().decode(), kw
    for kw in (dict(rgb=b.rgb + 4), dict(out=b.out_rgb + 8), dict(ws=b.ws + 4)):
        assert dev(**kw) == INV and "misaligned" in ftn.fn("last_error")().decode(), kw
    assert dev(ws=None) == INV and "null workspace" in ftn.fn("last_error")().decode()


def test_entries_that_run_on_the_gpu_report_no_device(ftn, lib):
    """No CPU fallback: valid arguments and no device -> FTN_ERR_NO_DEVICE, after every refusal"""
    if ftn.fn("device_count")() > 0:
        pytest.skip("a GPU is present")
    from fountain_amd.bloom import BloomParams
    b = Buffers()
    for kw in (dict(), dict(karis=True, threshold=1.0), dict(strength=0.0), dict(levels=0)):
        p = C.byref(BloomParams(ftn, **kw).desc)
        assert lib.ftn_bloom(b.rgb, b.w, b.h, p, b.out_rgb, -1) == NODEV
        assert lib.ftn_bloom_device(b.rgb, b.w, b.h, p, b.out_rgb, b.ws, None) == NODEV
    # no level, no workspace: a null one is then in order, and what follows is the missing device (with a device, over device memory:
    # tests/test_bloom.py)
    assert lib.ftn_bloom_device(b.rgb, b.w, b.h, C.byref(BloomParams(ftn, levels=0).desc), b.out_rgb, None, None) == NODEV
    assert lib.ftn_bloom_device(b.rgb, 1, 1, C.byref(BloomParams(ftn).desc), b.out_rgb, None, None) == NODEV
    assert b"no CPU fallback" in ftn.fn("last_error")()
    assert not b.store.any()


def test_cli_refusals(ftn, tmp_path):
    from fountain_amd import bloom, display, render
    scene = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")
    out = str(tmp_path / "a.exr")
    subs = (["--bloom-levels", "3"], ["--bloom-scatter", "0.5"], ["--bloom-threshold", "1"], ["--bloom-knee", "0.5"], ["--bloom-karis"])
    for extra in subs:
        assert render.main([scene, "-o", out, "--png"] + extra) == 2, extra                  # the sub-options belong to --bloom
        assert display.main([str(tmp_path / "in.exr")] + extra) == 2, extra
    assert render.main([scene, "-o", out, "--bloom"]) == 2                                   # --bloom belongs to --png
    assert render.main([scene, "-o", out, "--bloom", "0.1", "--bloom-karis"]) == 2
    assert render.main([scene, "-o", out, "--png", "--bloom", "--gpus", "2"]) == 2           # one GPU
    for bad in ("1.5", "-0.5", "nan"):
        assert render.main([scene, "-o", out, "--png", "--bloom", bad]) == 2, bad
        assert display.main([str(tmp_path / "in.exr"), "--bloom", bad]) == 2, bad
        assert bloom.main([str(tmp_path / "in.exr"), "--strength", bad]) == 2, bad
    # the sub-options' values are checked with the other refusals, before anything is rendered, read or written
    for bad in (["--bloom-levels", "13"], ["--bloom-levels", "-1"], ["--bloom-scatter", "1.5"], ["--bloom-scatter", "nan"], ["--bloom-threshold", "-1"],
                ["--bloom-threshold", "inf"], ["--bloom-knee", "2"], ["--bloom-knee", "-0.5"]):
        assert render.main([scene, "-o", out, "--png", "--bloom"] + bad) == 2, bad
        assert display.main([str(tmp_path / "in.exr"), "--bloom", "0.1"] + bad) == 2, bad
        assert bloom.main([str(tmp_path / "in.exr"), bad[0].replace("--bloom-", "--"), bad[1]]) == 2, bad
    assert bloom.main([str(tmp_path / "in.exr"), "-o", str(tmp_path / "out.png")]) == 2
    with pytest.raises(SystemExit):
        bloom.main([str(tmp_path / "in.exr"), "--levels", "two"])
    with pytest.raises(SystemExit):
        render.main([scene, "-o", out, "--png", "--bloom", "--bloom-levels", "two"])
    assert not list(tmp_path.iterdir())
