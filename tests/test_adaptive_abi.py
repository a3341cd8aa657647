"""The adaptive-sampling extension of the C ABI (include/fountain_hip_adaptive.h) without a GPU: the header, the ctypes mirror and the
library's exports agree; the layouts, versions and defaults; ftn_adaptive_converged against a float32 numpy restatement of the header's
criterion, bit for bit; the refusals, in the header's order, before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fountain_amd import _abi as A

from _moments_ref import criterion_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fountain_hip_adaptive.h")
F32 = np.float32


def adaptive_header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ftn_[a-z0-9_]+)\s*\(", src)))


def test_header_mirror_and_exports_agree(ftn):
    assert adaptive_header_functions() == sorted(A.ADAPTIVE_FUNCTIONS)
    for other in (A.DECLARED_FUNCTIONS, A.GBUFFER_FUNCTIONS, A.DENOISE_FUNCTIONS, A.MOMENTS_FUNCTIONS):
        assert not set(A.ADAPTIVE_FUNCTIONS) & set(other)
    for name in A.ADAPTIVE_FUNCTIONS:
        assert hasattr(ftn.lib, name), "libfountain_hip.so does not export %s" % name


def test_layouts():
    assert C.sizeof(A.ftn_adaptive_params) == 16 == A.SIZES["ftn_adaptive_params"]
    assert C.sizeof(A.ftn_adaptive_info) == 24 == A.SIZES["ftn_adaptive_info"]
    off = lambda T: {name: getattr(T, name).offset for name, _ in T._fields_}
    assert off(A.ftn_adaptive_params) == {"min_samples": 0, "step_samples": 4, "threshold": 8, "abs_floor": 12}
    assert off(A.ftn_adaptive_info) == {"rounds": 0, "tiles": 4, "tiles_at_max": 8, "_pad": 12, "pixel_samples": 16}


def test_versions(ftn):
    header = open(HEADER).read()
    assert int(re.search(r"#define\s+FTN_ADAPTIVE_ABI_VERSION\s+(\d+)", header).group(1)) == A.FTN_ADAPTIVE_ABI_VERSION == 1
    assert ftn.lib.ftn_adaptive_abi_version() == A.FTN_ADAPTIVE_ABI_VERSION
    assert ftn.lib.ftn_abi_version() == A.FTN_ABI_VERSION == 3          # the main ABI is unchanged by the extension
    assert ftn.lib.ftn_moments_abi_version() == A.FTN_MOMENTS_ABI_VERSION == 1


def test_defaults(ftn):
    from fountain_amd import adaptive
    p = A.ftn_adaptive_params(99, 99, 9.0, 9.0)
    ftn.lib.ftn_adaptive_params_default(C.byref(p))
    assert (p.min_samples, p.step_samples, p.threshold, p.abs_floor) == (8, 0, F32(0.05), F32(0.01))
    q = adaptive.params(ftn, threshold=0.2)
    assert (q.min_samples, q.step_samples, q.threshold, q.abs_floor) == (8, 0, F32(0.2), F32(0.01))
    with pytest.raises(TypeError):
        adaptive.params(ftn, thresold=0.2)


def _converged(ftn, pix, m, t, a):
    pix, m = np.ascontiguousarray(pix, F32), np.ascontiguousarray(m, F32)
    out = np.full(pix.shape[:-1], 7, np.uint8)
    prm = A.ftn_adaptive_params(8, 0, t, a)
    ftn.check(ftn.lib.ftn_adaptive_converged(pix.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), C.c_size_t(pix.size // 4),
                                             C.byref(prm), out.ctypes.data_as(C.c_void_p)))
    return out


def edge_cases(n=4096, seed=5):
    """random 2..64-sample pixels and then the edges: W = 0, 1, 2, 2^24; v = 0; mean = 0; NaN, inf and huge sums"""
    rng = np.random.default_rng(seed)
    W = rng.integers(2, 65, n).astype(F32)
    mean = rng.uniform(0.0, 2.0, n).astype(F32)
    rel = rng.uniform(0.0, 0.2, n).astype(F32)                             # relative standard error of the mean
    y = (mean * W).astype(F32)
    var_mean = ((rel * mean) ** 2).astype(F32)
    sq = (W * (var_mean * (W - 1) + mean * mean)).astype(F32)
    pix = np.stack([y * F32(0.9), y, y * F32(1.1), W], -1).astype(F32)
    m = np.stack([sq, sq, sq, sq], -1).astype(F32)
    k = 0

    def put(p, q):
        nonlocal k
        pix[k], m[k] = p, q
        k += 1
    put([0, 0, 0, 0], [0, 0, 0, 0])                      # W = 0: 0 / 0
    put([1, 1, 1, 1], [1, 1, 1, 1])                      # W = 1: inf
    put([2, 2, 2, 2], [2, 2, 2, 2])                      # W = 2, constant samples: v = 0
    put([0, 0, 0, 2], [0, 0, 0, 0])                      # W = 2, black: v = 0, mean = 0
    put([2 ** 24, 2 ** 24, 2 ** 24, 2 ** 24], [2 ** 24] * 4)
    put([3 * 2 ** 24, 2 ** 24, 1, 2 ** 24], [1, 1, 1, 1])
    put([0, 0, 0, 8], [0, 0, 0, 1e-6])                   # mean = 0, v > 0: only the floor decides
    put([0, np.nan, 0, 8], [1, 1, 1, 1])
    put([0, 1, 0, np.nan], [1, 1, 1, 1])
    put([0, 1, 0, 8], [1, 1, 1, np.nan])
    put([0, np.inf, 0, 8], [1, 1, 1, 1])
    put([0, 1, 0, np.inf], [1, 1, 1, 1])
    put([0, 1, 0, 8], [1, 1, 1, np.inf])
    put([0, 3e38, 0, 2], [1, 1, 1, 3e38])                # huge sums: mean * mean overflows
    put([0, 3e38, 0, 3e38], [1, 1, 1, 3e38])
    put([0, 1e19, 0, 4], [1, 1, 1, 1e38])
    put([0, 16, 0, 8], [0, 0, 0, 32 * (1 + 2 ** -20)])   # just above the cancellation edge
    return pix, m


@pytest.mark.parametrize("t,a", [(0.05, 0.01), (0.0, 0.01), (0.05, 0.0), (0.0, 0.0), (0.3, 0.5), (1e18, 0.0), (1e20, 1e20)])
def test_converged_bits(ftn, t, a):
    pix, m = edge_cases()
    out = _converged(ftn, pix, m, t, a)
    want = criterion_ref(pix, m, t, a)
    assert np.array_equal(out, want)
    assert set(np.unique(out)) <= {0, 1}
    assert out[0] == 0 and out[1] == 0                   # W = 0 and W = 1 never converge
    assert (out[7:13] == 0).all()                        # NaN and inf anywhere never converge
    if t > 0 and t < 1e10:
        assert out[2] == 1 and 0 < out.mean() < 1        # v = 0 always passes a finite bound; a mixed population
    if a == 0 and t < 1e10:
        assert out[6] == 0                               # a black pixel with any variance needs the floor


def test_converged_threshold_edge(ftn):
    """v exactly at the bound passes, one ulp above fails (v <= bound, no fused multiply-add)"""
    pix = np.array([[0, 4, 0, 4]] * 2, F32)             # mean 1
    t, a = F32(0.5), F32(0.0)
    bound = F32(t * t) * (F32(1) + F32(0))              # 0.25
    # v = (sq / 4 - 1) / 3 = bound -> sq = 4 * (3 bound + 1)
    sq = F32(4) * (F32(3) * bound + F32(1))
    m = np.array([[0, 0, 0, sq], [0, 0, 0, np.nextafter(sq, F32(np.inf))]], F32)
    out = _converged(ftn, pix, m, t, a)
    assert np.array_equal(out, criterion_ref(pix, m, t, a))
    assert list(out) == [1, 0]


def test_converged_refusals(ftn):
    pix, m = np.zeros((1, 4), F32), np.zeros((1, 4), F32)
    out = np.zeros(1, np.uint8)
    P, M, O = (x.ctypes.data_as(C.c_void_p) for x in (pix, m, out))
    for t, a in ((-0.1, 0.0), (np.nan, 0.0), (np.inf, 0.0), (0.1, -1.0), (0.1, np.nan), (0.1, np.inf)):
        prm = A.ftn_adaptive_params(8, 0, t, a)
        assert ftn.lib.ftn_adaptive_converged(P, M, C.c_size_t(1), C.byref(prm), O) == A.FTN_ERR_INVALID_ARGUMENT, (t, a)
    prm = A.ftn_adaptive_params(8, 0, 0.1, 0.0)
    assert ftn.lib.ftn_adaptive_converged(None, M, C.c_size_t(1), C.byref(prm), O) == A.FTN_ERR_INVALID_ARGUMENT
    assert ftn.lib.ftn_adaptive_converged(P, M, C.c_size_t(1), None, O) == A.FTN_ERR_INVALID_ARGUMENT
    assert ftn.lib.ftn_adaptive_converged(None, None, C.c_size_t(0), C.byref(prm), None) == A.FTN_OK


def _args(ftn, integrator=None, sampler=None, pipeline=A.FTN_PIPELINE_AUTO):
    from fountain_amd import PathIntegrator, PerspectiveCamera, RandomSampler, Film, Transform
    cam = PerspectiveCamera(ftn, Transform.identity(ftn), (8, 8))
    film = Film(ftn, (8, 8))
    smp = sampler or RandomSampler(16, 0, indexed=True)
    integ = integrator or PathIntegrator(3, 1.0)
    tr, opt, st = A.ftn_tile_range(), A.ftn_render_options(), A.ftn_stats()
    tr.stride, opt.device, opt.pipeline = 1, -1, pipeline
    keep = (cam, film, smp, integ, tr, opt)
    return [C.byref(cam.desc), C.byref(film.desc), C.byref(smp.desc), C.byref(integ.desc), C.byref(tr), C.byref(opt)], st, keep


class _Bufs:
    def __init__(self):
        self.px, self.mo, self.n = np.zeros((8, 8, 4), F32), np.zeros((8, 8, 4), F32), np.zeros((8, 8), np.uint32)
        self.P, self.M, self.N = (x.ctypes.data_as(C.c_void_p) for x in (self.px, self.mo, self.n))

    def untouched(self):
        return not self.px.any() and not self.mo.any() and not self.n.any()


def _both(ftn, scene, args, prm, b, st):
    info = A.ftn_adaptive_info()
    h = ftn.lib.ftn_render_adaptive(scene, *args, prm, b.P, b.M, b.N, C.byref(info), C.byref(st))
    d = ftn.lib.ftn_render_adaptive_device(scene, *args, prm, b.P, b.M, b.N, None, C.byref(info), C.byref(st))
    return h, d


def test_refusals_come_before_the_device(ftn):
    """null arguments, out-of-range parameters and partial sample ranges, then the tile-serial sampler, the megakernel and Whitted with
    more than 32 lights: refused on any machine, in the header's order, before the device check"""
    from fountain_amd import RandomSampler, WhittedIntegrator
    scene = (C.c_uint8 * 65536)()                        # stands in for a handle: the refusals never look at it (but for n_lights)
    S = C.byref(scene)
    b = _Bufs()
    good = C.byref(A.ftn_adaptive_params(8, 0, 0.05, 0.01))
    args, st, keep = _args(ftn)
    INV, UNS = A.FTN_ERR_INVALID_ARGUMENT, A.FTN_ERR_UNSUPPORTED
    assert ftn.lib.ftn_render_adaptive(None, *args, good, b.P, b.M, b.N, None, None) == INV
    assert ftn.lib.ftn_render_adaptive(S, *args, None, b.P, b.M, b.N, None, None) == INV
    assert ftn.lib.ftn_render_adaptive(S, *args, good, None, b.M, b.N, None, None) == INV
    assert ftn.lib.ftn_render_adaptive(S, *args, good, b.P, None, b.N, None, None) == INV
    assert ftn.lib.ftn_render_adaptive(S, *args, good, b.P, b.M, None, None, None) == INV
    assert ftn.lib.ftn_render_adaptive(S, *args[:3], None, *args[4:], good, b.P, b.M, b.N, None, None) == INV
    for i in (0, 1, 2):
        assert ftn.lib.ftn_render_adaptive_device(S, *args, good, *[None if k == i else x for k, x in enumerate((b.P, b.M, b.N))], None, None, None) == INV
    # parameters (N = 16)
    for p in ((1, 0, 0.05, 0.01), (0, 0, 0.05, 0.01), (17, 0, 0.05, 0.01), (8, 0, -0.05, 0.01), (8, 0, np.nan, 0.01), (8, 0, np.inf, 0.01),
              (8, 0, 0.05, -0.01), (8, 0, 0.05, np.nan), (8, 0, 0.05, np.inf)):
        assert _both(ftn, S, args, C.byref(A.ftn_adaptive_params(*p)), b, st) == (INV, INV), p
    # partial sample ranges
    for kw in (dict(first_sample=1), dict(sample_count=8), dict(first_sample=8, sample_count=8)):
        args, st, keep = _args(ftn, sampler=RandomSampler(16, 0, indexed=True, **kw))
        assert _both(ftn, S, args, good, b, st) == (INV, INV), kw
    # invalid comes before unsupported: a tile-serial sampler with a bad min_samples
    args, st, keep = _args(ftn, sampler=RandomSampler(16, 0))
    assert _both(ftn, S, args, C.byref(A.ftn_adaptive_params(1, 0, 0.05, 0.01)), b, st) == (INV, INV)
    for kw in (dict(sampler=RandomSampler(16, 0)), dict(pipeline=A.FTN_PIPELINE_MEGAKERNEL)):
        args, st, keep = _args(ftn, **kw)
        assert _both(ftn, S, args, good, b, st) == (UNS, UNS), kw
    assert b.untouched()


def test_render_without_gpu_reports_no_device(ftn):
    """No CPU fallback: valid arguments and no device give FTN_ERR_NO_DEVICE, with the buffers untouched"""
    if ftn.fn("device_count")() > 0:
        pytest.skip("a GPU is present")
    from fountain_amd import DirectLightingIntegrator, PathIntegrator, RandomSampler
    scene = (C.c_uint8 * 65536)()
    b = _Bufs()
    for integ in (PathIntegrator(3, 1.0), DirectLightingIntegrator(3)):
        for pl in (A.FTN_PIPELINE_AUTO, A.FTN_PIPELINE_WAVEFRONT):
            for smp in (RandomSampler(16, 0, indexed=True), RandomSampler(16, 0, indexed=True, sample_count=16)):
                args, st, keep = _args(ftn, integrator=integ, pipeline=pl, sampler=smp)
                assert _both(ftn, C.byref(scene), args, C.byref(A.ftn_adaptive_params(16, 3, 0.0, 0.0)), b, st) == (A.FTN_ERR_NO_DEVICE,) * 2
    assert b.untouched()


def test_oracle_backend_has_no_adaptive(orc):
    from fountain_amd import FountainError, adaptive
    with pytest.raises(FountainError) as e:
        adaptive.converged(orc, np.zeros((1, 4), F32), np.zeros((1, 4), F32), A.ftn_adaptive_params())
    assert "no oracle twin" in str(e.value)


def test_cli_refusals(tmp_path):
    from fountain_amd import render
    scene = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")
    out = str(tmp_path / "a.exr")
    for extra in (["--exact-stream"], ["--gbuffer"], ["--denoise"], ["--gpus", "2"]):
        assert render.main([scene, "-o", out, "--adaptive", "0.05"] + extra) == 2, extra
    assert render.main([scene, "-o", out, "--adaptive", "-1"]) == 2
    assert render.main([scene, "-o", out, "--adaptive", "inf"]) == 2
    assert render.main([scene, "-o", out, "--min-samples", "4"]) == 2
    # min_samples outside [2, samples per pixel], refused before the scene reaches a device
    assert render.main([scene, "-o", out, "--samples", "4", "--adaptive", "0.05", "--min-samples", "8"]) == 2
    assert render.main([scene, "-o", out, "--samples", "1", "--adaptive", "0.05"]) == 2
    assert render.main([scene, "-o", out, "--samples", "8", "--adaptive", "0.05", "--min-samples", "1"]) == 2
    assert not list(tmp_path.iterdir())
    assert render.spp_path("out.exr") == "out_spp.exr"
