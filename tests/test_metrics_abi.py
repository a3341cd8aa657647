"""The metrics extension of the C ABI (include/fountain_hip_metrics.h) without a GPU: the header, the ctypes mirror and the library's
exports agree; the layouts, the version and the defaults; the workspace formula; every refusal in the header's order for the host-buffer,
device and twin entries (each stage is tried with every later stage violated as well, the message must be its own, and no output byte
is written); then FTN_ERR_NO_DEVICE where there is no GPU; the oracle backend has no twin; the command lines' refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fountain_amd import _abi as A

import _metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fountain_hip_metrics.h")
F32 = np.float32
INV, NODEV = A.FTN_ERR_INVALID_ARGUMENT, A.FTN_ERR_NO_DEVICE


@pytest.fixture(scope="module")
def lib(ftn):
    from fountain_amd.metrics import _lib
    return _lib(ftn)


def header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ftn_[a-z0-9_]+)\s*\(", src)))


def test_header_mirror_and_exports_agree(ftn):
    import fountain_amd
    import fountain_amd.metrics as M
    assert header_functions() == sorted(A.METRICS_FUNCTIONS) == sorted(A.METRICS_PROTOTYPES)
    others = [getattr(A, name) for name in dir(A) if name.endswith("_FUNCTIONS") and name != "METRICS_FUNCTIONS"]
    assert len(others) >= 11
    for other in others:
        assert not set(A.METRICS_FUNCTIONS) & set(other)
    for name in A.METRICS_FUNCTIONS:
        assert hasattr(ftn.lib, name), "libfountain_hip.so does not export %s" % name
    # nothing of the stage is declared in the main header, whose functions all need an oracle twin
    assert "ftn_metrics" not in open(os.path.join(ROOT, "include", "fountain_hip.h")).read()
    for name in ("MetricsParams", "compare", "compare_cpu", "compare_device"):
        assert getattr(fountain_amd, name) is getattr(M, name) and name in fountain_amd.__all__
    assert callable(M.workspace_size)


def test_layouts_versions_and_constants(ftn, lib):
    offsets = lambda s: {name: getattr(s, name).offset for name, _ in s._fields_}
    assert C.sizeof(A.ftn_metrics_params) == 16 == A.SIZES["ftn_metrics_params"]
    assert offsets(A.ftn_metrics_params) == {"flags": 0, "peak": 4, "rel_eps": 8, "reserved": 12}
    assert C.sizeof(A.ftn_metrics_totals) == 112 == A.SIZES["ftn_metrics_totals"]
    assert offsets(A.ftn_metrics_totals) == {"sum": 0, "max_abs": 64, "max_abs_index": 72, "n_pixels": 80, "n_nonfinite": 88, "n_different": 96,
                                             "n_ssim_windows": 104}
    assert C.sizeof(A.ftn_metrics_result) == 136 == A.SIZES["ftn_metrics_result"]
    assert offsets(A.ftn_metrics_result) == {"mse": 0, "rmse": 8, "mae": 16, "rel_mse": 24, "smape": 32, "psnr": 40, "ssim": 48, "mse_rgb": 56, "max_abs": 80,
                                             "max_abs_index": 88, "n_pixels": 96, "n": 104, "n_nonfinite": 112, "n_different": 120, "n_ssim_windows": 128}
    header = open(HEADER).read()
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1))
    assert define("FTN_METRICS_ABI_VERSION") == A.FTN_METRICS_ABI_VERSION == 1 == lib.ftn_metrics_abi_version()
    assert define("FTN_METRICS_SSIM") == A.FTN_METRICS_SSIM == 1
    assert (define("FTN_METRICS_TILE"), define("FTN_METRICS_SUMS"), define("FTN_METRICS_SSIM_TAPS")) == (16, 8, 11) == (
        A.FTN_METRICS_TILE, A.FTN_METRICS_SUMS, A.FTN_METRICS_SSIM_TAPS)
    # the main ABI and the other extensions are unchanged
    assert ftn.lib.ftn_abi_version() == A.FTN_ABI_VERSION == 3
    assert ftn.lib.ftn_bloom_abi_version() == 1 and ftn.lib.ftn_display_abi_version() == 1 and ftn.lib.ftn_denoise_abi_version() == 1


def test_defaults(ftn, lib):
    from fountain_amd.metrics import MetricsParams
    d = MetricsParams(ftn).desc
    assert {k: getattr(d, k) for k, _ in d._fields_} == dict(flags=0, peak=1.0, rel_eps=float(F32(1e-2)), reserved=0)
    lib.ftn_metrics_params_default(None)                                  # ignored
    p = MetricsParams(ftn, ssim=True, peak=100.0)
    assert (p.desc.flags, p.desc.peak) == (1, 100.0)
    assert MetricsParams(ftn, ssim=False).desc.flags == 0
    with pytest.raises(TypeError):
        MetricsParams(ftn, sigma=1.5)


def test_oracle_backend_has_no_metrics_stage(orc):
    from fountain_amd import FountainError
    from fountain_amd.metrics import MetricsParams
    with pytest.raises(FountainError) as e:
        MetricsParams(orc)
    assert "no oracle twin" in str(e.value)


def test_workspace_formula(ftn, lib):
    from fountain_amd.metrics import workspace_size
    for w, h in ((1, 1), (16, 16), (17, 16), (16, 17), (255, 257), (256, 256), (257, 256), (4096, 4096), (4097, 4096), (5000, 3), (65536, 32767), (46340, 46340)):
        for flags in (0, 1):
            assert workspace_size(ftn, w, h, flags) == R.workspace_bytes(w, h), (w, h)
    assert workspace_size(ftn, 1, 1) == 88 + 8                          # one record, to 16 bytes
    assert workspace_size(ftn, 256, 256) == 88 * 256                    # 256 tiles: one level
    assert workspace_size(ftn, 272, 256) == 88 * (272 + 2)              # 272 tiles: two records above them
    assert workspace_size(ftn, 4096, 4096) == 88 * (65536 + 256)
    n = C.c_size_t(77)
    assert lib.ftn_metrics_workspace_size(8, 8, 0, None) == INV and "null" in ftn.fn("last_error")().decode()
    assert lib.ftn_metrics_workspace_size(0, 8, 2, C.byref(n)) == INV and "positive" in ftn.fn("last_error")().decode()
    assert lib.ftn_metrics_workspace_size(65536, 32768, 2, C.byref(n)) == INV and "2^31" in ftn.fn("last_error")().decode()
    assert lib.ftn_metrics_workspace_size(8, 8, 2, C.byref(n)) == INV and "flags bits" in ftn.fn("last_error")().decode()
    assert n.value == 77


def test_ssim_weights(ftn, lib):
    from fountain_amd.metrics import ssim_weights
    g = ssim_weights(ftn)
    assert g.shape == (11,) and np.array_equal(g, g[::-1]) and abs(g.sum() - 1.0) < 1e-15
    assert np.abs(g - R.weights()).max() <= 2.0 ** -52                   # Python's exp against the library's
    assert lib.ftn_metrics_ssim_weights(None) == INV


# ------------------------------------------------------------------ refusals, in the header's order
# (stage, what to violate, the words its message must hold); "p." names a field of the parameters
STAGES = [("null", None, "null argument"), ("size", None, "positive"),
          ("p.flags", 2, "flags bits"), ("p.reserved", 1, "reserved"), ("p.peak", float("nan"), "finite and above 0"),
          ("small", None, "11 x 11"), ("map without flag", None, "needs FTN_METRICS_SSIM"),
          ("null workspace", None, "null workspace"), ("overlap", None, "overlaps"), ("align", None, "misaligned")]


class Buffers:
    """host memory standing in for device memory as well: no refusal looks behind a pointer"""

    def __init__(self, w=5, h=7):
        self.w, self.h = w, h
        up = lambda n: 16 * ((n + 15) // 16)
        sizes = [up(12 * w * h), up(12 * w * h), 144, 112, up(4 * w * h), up(4 * w * h), up(64 * R.tiles(w, h)[0] * R.tiles(w, h)[1]), R.workspace_bytes(w, h)]
        sizes = [n + 16 for n in sizes]                                    # room to shift a buffer off its alignment
        self.store = np.zeros(sum(sizes) // 4 + 64, F32)
        base = self.store.ctypes.data
        base += (-base) % 16
        at = [base + sum(sizes[:i]) for i in range(len(sizes))]
        self.test, self.ref, self.result, self.totals, self.err, self.ssim, self.tiles, self.ws = at
        self.n_rgb = 12 * w * h


def _violated(ftn, entry, first, stages):
    """arguments of `entry` with every stage from `first` on violated ("small" and "map without flag" exclude each other: the first
    needs the flag, the second its absence; the map is there in both)"""
    from fountain_amd.metrics import MetricsParams
    on = stages[stages.index(first):]
    is_on = lambda name: any(s[0] == name for s in on)
    b = Buffers()
    p = MetricsParams(ftn).desc
    for name, value, _ in on:
        if name.startswith("p."):
            setattr(p, name[2:], value)
    if is_on("small"):
        p.flags |= A.FTN_METRICS_SSIM
    w = 0 if is_on("size") else b.w
    test = None if is_on("null") else b.test
    err = b.test + 16 if is_on("overlap") else (b.err + 4 if is_on("align") else b.err)
    ws = None if is_on("null workspace") else (b.ws + 4 if is_on("align") else b.ws)
    ssim = b.ssim if is_on("map without flag") else None
    P = C.byref(p)
    return {"metrics": (test, b.ref, w, b.h, P, b.result, b.totals, err, ssim, b.tiles, -1),
            "metrics_device": (test, b.ref, w, b.h, P, b.totals, err, ssim, b.tiles, ws, None),
            "metrics_cpu": (test, b.ref, w, b.h, P, b.result, b.totals, err, ssim, b.tiles)}[entry], b


ENTRY_STAGES = {"metrics": STAGES[:7], "metrics_device": STAGES, "metrics_cpu": STAGES[:7]}


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
    from fountain_amd.metrics import MetricsParams
    b = Buffers(12, 13)

    def P(**fields):
        d = MetricsParams(ftn).desc
        for k, v in fields.items():
            setattr(d, k, v)
        return C.byref(d)
    cpu = lambda p, w=b.w, h=b.h, test=b.test, ref=b.ref, result=b.result, ssim=None: lib.ftn_metrics_cpu(test, ref, w, h, p, result, None, None, ssim, None)
    assert cpu(P()) == 0 and cpu(P(flags=1)) == 0 and cpu(P(flags=1), ssim=b.ssim) == 0 and cpu(P(), test=b.test, ref=b.test) == 0
    assert cpu(None) == INV and cpu(P(), result=None) == INV and cpu(P(), test=None) == INV and cpu(P(), ref=None) == INV
    assert cpu(P(), w=-1) == INV and cpu(P(), h=0) == INV
    assert cpu(P(), w=65536, h=32768) == INV and "2^31" in ftn.fn("last_error")().decode()
    for kw in (dict(flags=0x80000000), dict(flags=3), dict(reserved=0xffffffff), dict(peak=float("nan")), dict(peak=float("inf")), dict(peak=0.0),
               dict(peak=-1.0), dict(rel_eps=float("nan")), dict(rel_eps=float("inf")), dict(rel_eps=0.0), dict(rel_eps=-1e-2)):
        assert cpu(P(**kw)) == INV, kw
    for kw in (dict(peak=1e30), dict(peak=1e-30), dict(rel_eps=1e-30), dict(rel_eps=1e30)):
        assert cpu(P(**kw)) == 0, kw
    assert cpu(P(flags=1), w=10) == INV and "11 x 11" in ftn.fn("last_error")().decode()
    assert cpu(P(flags=1), w=11, h=10) == INV and cpu(P(flags=1), w=11, h=11) == 0
    assert cpu(P(), ssim=b.ssim) == INV and "needs FTN_METRICS_SSIM" in ftn.fn("last_error")().decode()
    # the resolve
    t = A.ftn_metrics_totals()
    r = A.ftn_metrics_result()
    assert lib.ftn_metrics_resolve(None, P(), C.byref(r)) == INV and lib.ftn_metrics_resolve(C.byref(t), None, C.byref(r)) == INV
    assert lib.ftn_metrics_resolve(C.byref(t), P(), None) == INV and lib.ftn_metrics_resolve(C.byref(t), P(peak=0.0), C.byref(r)) == INV
    assert lib.ftn_metrics_resolve(C.byref(t), P(), C.byref(r)) == 0 and np.isnan(r.mse) and np.isnan(r.psnr) and np.isnan(r.ssim) and np.isnan(r.max_abs)
    # the device path: every output against the inputs and against the outputs after it; each buffer's alignment
    dev = lambda test=b.test, ref=b.ref, tot=b.totals, err=b.err, ssim=None, tiles=b.tiles, ws=b.ws, p=None: lib.ftn_metrics_device(
        test, ref, b.w, b.h, p or P(), tot, err, ssim, tiles, ws, None)
    for kw in (dict(tot=b.test), dict(tot=b.ref + b.n_rgb - 16), dict(err=b.test + b.n_rgb - 16), dict(err=b.ref), dict(tiles=b.ref), dict(ws=b.test),
               dict(ws=b.ref + b.n_rgb - 16), dict(ssim=b.test, p=P(flags=1))):
        assert dev(**kw) == INV and "overlaps an input" in ftn.fn("last_error")().decode(), kw
    for kw in (dict(err=b.totals), dict(tiles=b.err), dict(ws=b.tiles), dict(ws=b.totals + 96), dict(ws=b.tiles - 16), dict(ssim=b.err, p=P(flags=1)), dict(tot=b.ws)):
        assert dev(**kw) == INV and "outputs and the workspace overlap" in ftn.fn("last_error")().decode(), kw
    for kw in (dict(test=b.test + 4), dict(ref=b.ref + 8), dict(tot=b.result + 8), dict(err=b.err + 4), dict(tiles=b.tiles + 8), dict(ws=b.ws + 8),
               dict(ssim=b.ssim + 4, p=P(flags=1))):
        assert dev(**kw) == INV and "misaligned" in ftn.fn("last_error")().decode(), kw
    assert dev(ws=None) == INV and "null workspace" in ftn.fn("last_error")().decode()
    assert dev(tot=None) == INV and "null argument" in ftn.fn("last_error")().decode()


def test_entries_that_run_on_the_gpu_report_no_device(ftn, lib):
    """No CPU fallback: valid arguments and no device -> FTN_ERR_NO_DEVICE, after every refusal"""
    if ftn.fn("device_count")() > 0:
        pytest.skip("a GPU is present")
    from fountain_amd.metrics import MetricsParams
    b = Buffers(12, 13)
    for kw in (dict(), dict(ssim=True), dict(ssim=True, peak=100.0)):
        p = C.byref(MetricsParams(ftn, **kw).desc)
        ssim = b.ssim if kw else None
        assert lib.ftn_metrics(b.test, b.ref, b.w, b.h, p, b.result, b.totals, b.err, ssim, b.tiles, -1) == NODEV
        assert lib.ftn_metrics(b.test, b.test, b.w, b.h, p, b.result, None, None, None, None, 0) == NODEV
        assert lib.ftn_metrics_device(b.test, b.ref, b.w, b.h, p, b.totals, b.err, ssim, b.tiles, b.ws, None) == NODEV
        assert lib.ftn_metrics_device(b.test, b.test, b.w, b.h, p, b.totals, None, None, None, b.ws, None) == NODEV
    assert b"no CPU fallback" in ftn.fn("last_error")()
    assert not b.store.any()


def test_cli_refusals(ftn, tmp_path):
    from fountain_amd import metrics, render
    from fountain_amd.api import write_exr
    scene = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")
    work, refs = tmp_path / "work", tmp_path / "refs"
    work.mkdir()
    refs.mkdir()
    write_exr(str(refs / "a.exr"), np.zeros((12, 13, 3), F32), ftn)
    write_exr(str(refs / "b.exr"), np.zeros((13, 12, 3), F32), ftn)
    write_exr(str(refs / "small.exr"), np.zeros((10, 64, 3), F32), ftn)
    (refs / "junk.exr").write_bytes(b"not an image")
    a, b = str(refs / "a.exr"), str(refs / "b.exr")
    out = str(work / "map.exr")
    M = lambda *args: metrics.main(list(args) + ["--cpu"])
    assert M(str(work / "none.exr"), a) == 2 and M(a, str(work / "none.exr")) == 2 and M(a, str(refs / "junk.exr")) == 2
    assert M(a, b, "--error-map", out, "--tile-map", str(work / "t.exr")) == 2                       # sizes that differ: nothing is written
    assert M(a, a, "--ssim-map", out) == 2                                                            # belongs to --ssim
    assert M(a, a, "--error-map", str(work / "map.png")) == 2 and M(a, a, "--tile-map", str(work / "map")) == 2
    assert M(str(refs / "small.exr"), str(refs / "small.exr"), "--ssim", "--error-map", out) == 2     # 10 rows: no window
    for bad in ("rmse", "rmse=", "rmse=x", "rmse=nan", "psnr=3", "ssim=0.5", "=1"):
        assert M(a, a, "--fail-above", bad, "--error-map", out) == 2, bad
    for bad in (["--peak", "0"], ["--peak", "nan"], ["--peak", "inf"], ["--rel-eps", "-1"], ["--rel-eps", "0"]):
        assert M(a, a, "--error-map", out, *bad) == 2, bad
    with pytest.raises(SystemExit):
        M(a)
    with pytest.raises(SystemExit):
        M(a, a, "--peak", "high")
    # fountain_amd.render --compare-to: refused before anything is rendered (none of these needs a GPU)
    img = str(work / "img.exr")
    assert render.main([scene, "-o", img, "--ssim"]) == 2                                              # belongs to --compare-to
    assert render.main([scene, "-o", img, "--compare-to", str(work / "none.exr")]) == 2                # missing
    assert render.main([scene, "-o", img, "--compare-to", scene]) == 2                                 # not .exr
    assert render.main([scene, "-o", img, "--compare-to", a]) == 2                                     # 13 x 12, the film is 64 x 64
    assert render.main([scene, "-o", img, "--compare-to", str(refs / "small.exr")]) == 2
    assert render.main([scene, "-o", img, "--compare-to", str(refs / "junk.exr")]) == 2
    assert render.main([scene, "-o", img, "--compare-to", a, "--gpus", "2"]) == 2 and render.main([scene, "-o", img, "--compare-to", a, "--gpus", "1"]) == 2
    assert not list(work.iterdir())
    assert sorted(f.name for f in refs.iterdir()) == ["a.exr", "b.exr", "junk.exr", "small.exr"]
