"""The display extension of the C ABI (include/fountain_hip_display.h) without a GPU: the header, the ctypes mirror and the library's
exports agree; the layout, the version and the defaults; every refusal in the header's order for the host-buffer, device and twin
entries (each stage is tried with every later stage violated as well, and the message must be its own); then FTN_ERR_NO_DEVICE where
there is no GPU; the command lines' refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fountain_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fountain_hip_display.h")
F32 = np.float32
INV, NODEV = A.FTN_ERR_INVALID_ARGUMENT, A.FTN_ERR_NO_DEVICE


@pytest.fixture(scope="module")
def lib(ftn):
    from fountain_amd.display import _lib
    return _lib(ftn)


def header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ftn_[a-z0-9_]+)\s*\(", src)))


def test_header_mirror_and_exports_agree(ftn):
    import fountain_amd
    assert header_functions() == sorted(A.DISPLAY_FUNCTIONS) == sorted(A.DISPLAY_PROTOTYPES)
    for other in (A.DECLARED_FUNCTIONS, A.GBUFFER_FUNCTIONS, A.DENOISE_FUNCTIONS, A.DENOISE_GUIDED_FUNCTIONS, A.MOMENTS_FUNCTIONS, A.ADAPTIVE_FUNCTIONS,
                  A.TEMPORAL_FUNCTIONS, A.FILTER_FUNCTIONS):
        assert not set(A.DISPLAY_FUNCTIONS) & set(other)
    for name in A.DISPLAY_FUNCTIONS:
        assert hasattr(ftn.lib, name), "libfountain_hip.so does not export %s" % name
    # nothing of the display stage is declared in the main header, whose functions all need an oracle twin
    main = open(os.path.join(ROOT, "include", "fountain_hip.h")).read()
    assert "ftn_display" not in main and "ftn_png" not in main
    import fountain_amd.display as D
    assert fountain_amd.DisplayParams is D.DisplayParams and fountain_amd.write_png is D.write_png
    assert "DisplayParams" in fountain_amd.__all__ and "write_png" in fountain_amd.__all__


def test_layout_versions_and_constants(ftn, lib):
    assert C.sizeof(A.ftn_display_params) == 48 == A.SIZES["ftn_display_params"]
    assert C.sizeof(A.ftn_display_info) == 32 == A.SIZES["ftn_display_info"]
    off = lambda T: {name: getattr(T, name).offset for name, _ in T._fields_}
    assert off(A.ftn_display_params) == {"tonemap": 0, "transfer": 4, "flags": 8, "reserved": 12, "ev": 16, "key": 20, "white": 24, "gamma": 28,
                                         "p_lo": 32, "p_hi": 36, "min_ev": 40, "max_ev": 44}
    assert off(A.ftn_display_info) == {"scale": 0, "flags": 4, "avg_log2": 8, "count_bins": 16, "count_invalid": 20, "count_below": 24, "count_above": 28}
    header = open(HEADER).read()
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1))
    assert define("FTN_DISPLAY_ABI_VERSION") == A.FTN_DISPLAY_ABI_VERSION == 1 == lib.ftn_display_abi_version()
    for name in ("FTN_DISPLAY_HIST_BINS", "FTN_DISPLAY_HIST_INVALID", "FTN_DISPLAY_HIST_BELOW", "FTN_DISPLAY_HIST_ABOVE", "FTN_DISPLAY_HIST_WORDS",
                 "FTN_DISPLAY_DITHER", "FTN_DISPLAY_AUTO_EXPOSURE", "FTN_DISPLAY_INFO_EMPTY", "FTN_PNG_GAMA"):
        assert define(name) == getattr(A, name), name
    assert A.FTN_DISPLAY_HIST_WORDS * 4 % 16 == 0
    enum = {k: int(v) for k, v in re.findall(r"(FTN_DISPLAY_(?:TONEMAP|TRANSFER)_[A-Z]+) = (\d+)", header)}
    assert enum == {k: getattr(A, k) for k in enum} and len(enum) == 7
    # the main ABI and the other extensions are unchanged
    assert ftn.lib.ftn_abi_version() == A.FTN_ABI_VERSION == 3
    assert ftn.lib.ftn_filter_abi_version() == 1 and ftn.lib.ftn_temporal_abi_version() == 1 and ftn.lib.ftn_denoise_abi_version() == 1


def test_defaults(ftn, lib):
    from fountain_amd.display import DisplayParams
    d = DisplayParams(ftn).desc
    got = {k: getattr(d, k) for k, _ in d._fields_}
    want = dict(tonemap=A.FTN_DISPLAY_TONEMAP_ACES, transfer=A.FTN_DISPLAY_TRANSFER_SRGB, flags=0, reserved=0, ev=0.0, key=float(F32(0.18)),
                white=float(F32(11.2)), gamma=float(F32(2.2)), p_lo=float(F32(0.10)), p_hi=float(F32(0.95)), min_ev=-16.0, max_ev=16.0)
    assert got == want
    lib.ftn_display_params_default(None)                                  # ignored
    p = DisplayParams(ftn, tonemap="hable", transfer="gamma", dither=True, auto_exposure=True, gamma=2.4, key=0.25)
    assert (p.desc.tonemap, p.desc.transfer, p.desc.flags) == (3, 1, 3) and p.desc.gamma == F32(2.4) and p.png_gamma == float(F32(2.4))
    assert DisplayParams(ftn).png_gamma is None and DisplayParams(ftn, transfer="linear").png_gamma == 1.0
    with pytest.raises(ValueError):
        DisplayParams(ftn, tonemap="filmic")
    with pytest.raises(TypeError):
        DisplayParams(ftn, exposure=1.0)


def test_oracle_backend_has_no_display_stage(orc):
    from fountain_amd import FountainError
    from fountain_amd.display import DisplayParams
    with pytest.raises(FountainError) as e:
        DisplayParams(orc)
    assert "no oracle twin" in str(e.value)


# ------------------------------------------------------------------ refusals, in the header's order
# (stage, what to violate, the words its message must hold); "p." names a field of the parameters
STAGES = [("null", None, "null"), ("size", None, "positive"),
          ("p.tonemap", 4, "tonemap"), ("p.transfer", 3, "transfer"), ("p.flags", 4, "flags bits"), ("p.reserved", 1, "reserved"),
          ("p.ev", float("nan"), "ev, key"), ("p.key", 0.0, "above 0"), ("p.p_hi", 0.05, "percentiles"), ("p.min_ev", 17.0, "min_ev"),
          ("scale", float("inf"), "scale"), ("overlap", None, "overlaps"), ("align", None, "misaligned")]


class Buffers:
    """host memory standing in for device memory as well: no refusal looks behind a pointer"""

    def __init__(self, w=5, h=7):
        self.w, self.h = w, h
        self.store = np.zeros(16 * w * h + 1024, F32)               # rgb | out_rgb | out_rgba8 | hist, each 16-byte aligned
        base = self.store.ctypes.data
        base += (-base) % 16
        n = w * h
        self.rgb, self.out_rgb, self.out8 = base, base + 16 * ((12 * n + 15) // 16), base + 2 * 16 * ((12 * n + 15) // 16)
        self.hist = self.out8 + 16 * ((4 * n + 15) // 16)


def _violated(ftn, entry, first, stages):
    """arguments of `entry` with every stage from `first` on violated"""
    from fountain_amd.display import DisplayParams
    on = [s for s in stages[stages.index(first):]]
    is_on = lambda name: any(s[0] == name for s in on)
    b = Buffers()
    p = DisplayParams(ftn).desc
    for name, value, _ in on:
        if name.startswith("p."):
            setattr(p, name[2:], value)
    w = 0 if is_on("size") else b.w
    rgb = None if is_on("null") else b.rgb
    scale = float("inf") if is_on("scale") else 1.0
    out_rgb = b.rgb + 16 if is_on("overlap") else b.out_rgb
    out8 = b.out8 + 4 if is_on("align") else b.out8
    hist = b.rgb if is_on("overlap") else (b.hist + 4 if is_on("align") else b.hist)
    P = C.byref(p)
    return {"encode": (rgb, w, b.h, P, scale, out_rgb, out8, -1), "encode_device": (rgb, w, b.h, P, scale, out_rgb, out8, None),
            "encode_cpu": (rgb, w, b.h, P, scale, out_rgb, out8), "display": (rgb, w, b.h, P, out_rgb, out8, None, -1),
            "histogram": (rgb, w, b.h, hist, -1), "histogram_device": (rgb, w, b.h, hist, None), "histogram_cpu": (rgb, w, b.h, hist),
            "exposure": (None if is_on("null") else hist, P, C.byref(A.ftn_display_info()))}[entry], b


PARAM_STAGES = [s for s in STAGES if s[0].startswith("p.")]
ENTRY_STAGES = {
    "encode": STAGES[:2] + PARAM_STAGES + [STAGES[10]],
    "encode_device": STAGES,
    "encode_cpu": STAGES[:2] + PARAM_STAGES + [STAGES[10]],
    "display": STAGES[:2] + PARAM_STAGES,
    "histogram": STAGES[:2],
    "histogram_device": STAGES[:2] + STAGES[11:],
    "histogram_cpu": STAGES[:2],
    "exposure": STAGES[:1] + PARAM_STAGES,
}


@pytest.mark.parametrize("entry", sorted(ENTRY_STAGES))
def test_refusals_in_order(ftn, lib, entry):
    fn = getattr(lib, "ftn_display_" + entry) if entry != "display" else lib.ftn_display
    stages = ENTRY_STAGES[entry]
    for first in stages:
        args, keep = _violated(ftn, entry, first, stages)
        if entry == "exposure" and first[0] == "null":
            args[1]._obj.flags = A.FTN_DISPLAY_AUTO_EXPOSURE | 4            # a null histogram is refused in automatic mode only
        assert fn(*args) == INV, (entry, first[0])
        assert first[2] in ftn.fn("last_error")().decode(), (entry, first[0], ftn.fn("last_error")())
        assert not keep.store.any()


def test_further_refusals(ftn, lib):
    from fountain_amd.display import DisplayParams
    b = Buffers()
    def P(**fields):
        d = DisplayParams(ftn).desc
        for k, v in fields.items():
            setattr(d, k, v)
        return C.byref(d)
    enc = lambda p, scale=1.0, w=b.w, h=b.h, rgb=b.rgb, out8=b.out8: lib.ftn_display_encode_cpu(rgb, w, h, p, scale, None, out8)
    assert enc(P()) == 0                                                           # out_rgb may be null
    assert enc(None) == INV and enc(P(), out8=None) == INV
    assert enc(P(), w=-1) == INV and enc(P(), h=0) == INV
    assert enc(P(), w=65536, h=32768) == INV and "2^31" in ftn.fn("last_error")().decode()
    for kw in (dict(ev=float("inf")), dict(key=float("nan")), dict(white=float("inf")), dict(gamma=float("-inf")), dict(key=-1.0), dict(white=0.0),
               dict(gamma=0.0), dict(gamma=-2.2), dict(p_lo=-0.1), dict(p_hi=1.5), dict(p_lo=0.95, p_hi=0.10), dict(p_lo=float("nan")),
               dict(min_ev=float("nan")), dict(max_ev=float("nan")), dict(tonemap=0xffffffff), dict(transfer=0xffffffff), dict(flags=0x80000000)):
        assert enc(P(**kw)) == INV, kw
    assert enc(P(), scale=-1.0) == INV and enc(P(), scale=float("nan")) == INV and enc(P(), scale=0.0) == 0
    assert enc(P(min_ev=3.0, max_ev=3.0, p_lo=0.0, p_hi=1.0)) == 0
    # the device path: each output against the input and against the other output; each buffer's alignment
    dev = lambda rgb=b.rgb, out_rgb=b.out_rgb, out8=b.out8: lib.ftn_display_encode_device(rgb, b.w, b.h, P(), 1.0, out_rgb, out8, None)
    n = b.w * b.h
    for kw in (dict(out8=b.rgb), dict(out8=b.rgb + 12 * n - 16), dict(out_rgb=b.rgb), dict(out_rgb=b.out8), dict(out_rgb=b.out8 - 16)):
        assert dev(**kw) == INV and "overlaps" in ftn.fn("last_error")().decode(), kw
    for kw in (dict(rgb=b.rgb + 4), dict(out_rgb=b.out_rgb + 8), dict(out8=b.out8 + 4)):
        assert dev(**kw) == INV and "misaligned" in ftn.fn("last_error")().decode(), kw
    assert lib.ftn_display_histogram_device(b.rgb + 4, b.w, b.h, b.hist, None) == INV
    assert lib.ftn_display_histogram_device(b.rgb, b.w, b.h, b.rgb + 16, None) == INV and "overlaps" in ftn.fn("last_error")().decode()
    # manual mode needs no histogram; automatic mode does
    info = A.ftn_display_info()
    assert lib.ftn_display_exposure(None, P(ev=1.0), C.byref(info)) == 0 and info.scale == 2.0 and info.count_bins == 0
    assert lib.ftn_display_exposure(None, P(flags=A.FTN_DISPLAY_AUTO_EXPOSURE), C.byref(info)) == INV
    assert lib.ftn_display_exposure(b.hist, P(), None) == INV


def test_entries_that_run_on_the_gpu_report_no_device(ftn, lib):
    """No CPU fallback: valid arguments and no device -> FTN_ERR_NO_DEVICE, after every refusal"""
    if ftn.fn("device_count")() > 0:
        pytest.skip("a GPU is present")
    from fountain_amd.display import DisplayParams
    b = Buffers()
    for kw in (dict(), dict(auto_exposure=True), dict(tonemap="reinhard", transfer="gamma", dither=True)):
        p = C.byref(DisplayParams(ftn, **kw).desc)
        assert lib.ftn_display_encode(b.rgb, b.w, b.h, p, 1.0, b.out_rgb, b.out8, -1) == NODEV
        assert lib.ftn_display_encode_device(b.rgb, b.w, b.h, p, 1.0, None, b.out8, None) == NODEV
        assert lib.ftn_display(b.rgb, b.w, b.h, p, None, b.out8, None, -1) == NODEV
    assert lib.ftn_display_histogram(b.rgb, b.w, b.h, b.hist, -1) == NODEV
    assert lib.ftn_display_histogram_device(b.rgb, b.w, b.h, b.hist, None) == NODEV
    assert b"no CPU fallback" in ftn.fn("last_error")()
    assert not b.store.any()


def test_png_refusals(ftn, lib, tmp_path):
    px = np.zeros((7, 5), np.uint32)
    P = px.ctypes.data_as(C.c_void_p)
    path = os.fsencode(str(tmp_path / "a.png"))
    assert lib.ftn_png_write(None, P, 5, 7, 0) == INV and lib.ftn_png_write(path, None, 5, 7, 0) == INV
    assert lib.ftn_png_write(path, P, 0, 7, 0) == INV and lib.ftn_png_write(path, P, 5, 0, 0) == INV
    assert lib.ftn_png_write(path, P, 65536, 32768, 0) == INV
    for flags in (2, 0x80, 45455 << 8, A.FTN_PNG_GAMA):                          # unknown bits; a value without the flag; the flag without a value
        assert lib.ftn_png_write(path, P, 5, 7, flags) == INV, flags
    assert not list(tmp_path.iterdir())
    assert lib.ftn_png_write(os.fsencode(str(tmp_path / "no_such_directory" / "a.png")), P, 5, 7, 0) == INV
    assert b"cannot create" in ftn.fn("last_error")()
    assert lib.ftn_png_write(path, P, 5, 7, (45455 << 8) | A.FTN_PNG_GAMA) == 0 and os.path.getsize(path) > 8


def test_cli_refusals(ftn, tmp_path):
    from fountain_amd import display, render
    scene = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")
    out = str(tmp_path / "a.exr")
    for extra in (["--dither"], ["--auto-exposure"], ["--exposure", "1"], ["--tonemap", "aces"], ["--transfer", "srgb"], ["--gamma", "2.2"]):
        assert render.main([scene, "-o", out] + extra) == 2, extra                           # the display options belong to --png
    assert render.main([scene, "-o", out, "--png", "--gpus", "2"]) == 2
    assert render.main([scene, "-o", out, "--png", "--gamma", "2.2"]) == 2                   # --gamma belongs to --transfer gamma
    assert render.main([scene, "-o", out, "--png", "--transfer", "srgb", "--gamma", "2.2"]) == 2
    for bad in (["--png", "--exposure", "1", "--auto-exposure"], ["--png", "--tonemap", "filmic"], ["--png", "--transfer", "pq"]):
        with pytest.raises(SystemExit):
            render.main([scene, "-o", out] + bad)
    exr = str(tmp_path / "in.exr")
    assert display.main([exr, "-o", str(tmp_path / "out.jpg")]) == 2
    assert display.main([exr, "-o", str(tmp_path / "out.png"), "--gamma", "2.2"]) == 2
    with pytest.raises(SystemExit):
        display.main([exr, "--exposure", "1", "--auto-exposure"])
    assert not list(tmp_path.iterdir())
