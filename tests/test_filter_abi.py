"""The reconstruction-filter extension of the C ABI (include/fountain_hip_filter.h) without a GPU: the header, the ctypes mirror and the
library's exports agree; the layout, the version and every kind's defaults; ftn_filter_table against a float64 numpy restatement of
PBRT v3's formulas; every refusal, in the header's order, for the host twin and the render entries, then FTN_ERR_NO_DEVICE where there is
no GPU; the loader's getter; the command line's refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fountain_amd import _abi as A

import _filter_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fountain_hip_filter.h")
F32 = np.float32
INV, UNS, NODEV = A.FTN_ERR_INVALID_ARGUMENT, A.FTN_ERR_UNSUPPORTED, A.FTN_ERR_NO_DEVICE


def filter_header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ftn_[a-z0-9_]+)\s*\(", src)))


def test_header_mirror_and_exports_agree(ftn):
    import fountain_amd
    assert filter_header_functions() == sorted(A.FILTER_FUNCTIONS) == sorted(A.FILTER_PROTOTYPES)
    for other in (A.DECLARED_FUNCTIONS, A.GBUFFER_FUNCTIONS, A.DENOISE_FUNCTIONS, A.DENOISE_GUIDED_FUNCTIONS, A.MOMENTS_FUNCTIONS, A.ADAPTIVE_FUNCTIONS,
                  A.TEMPORAL_FUNCTIONS):
        assert not set(A.FILTER_FUNCTIONS) & set(other)
    for name in A.FILTER_FUNCTIONS:
        assert hasattr(ftn.lib, name), "libfountain_hip.so does not export %s" % name
    assert fountain_amd.Filter is fountain_amd.filters.Filter and fountain_amd.render_filtered is fountain_amd.filters.render_filtered
    assert "Filter" in fountain_amd.__all__ and "render_filtered" in fountain_amd.__all__


def test_layout_and_versions(ftn):
    assert C.sizeof(A.ftn_filter_desc) == 32 == A.SIZES["ftn_filter_desc"]
    offsets = {name: getattr(A.ftn_filter_desc, name).offset for name, _ in A.ftn_filter_desc._fields_}
    assert offsets == {"kind": 0, "radius": 4, "param": 12, "reserved": 20}
    header = open(HEADER).read()
    assert int(re.search(r"#define\s+FTN_FILTER_ABI_VERSION\s+(\d+)", header).group(1)) == A.FTN_FILTER_ABI_VERSION == 1
    assert ftn.lib.ftn_filter_abi_version() == A.FTN_FILTER_ABI_VERSION
    assert ftn.lib.ftn_abi_version() == A.FTN_ABI_VERSION == 3          # the main ABI and the other extensions are unchanged
    assert ftn.lib.ftn_moments_abi_version() == 1 and ftn.lib.ftn_temporal_abi_version() == 1
    enum = dict(re.findall(r"(FTN_FILTER_[A-Z]+) = (\d+)", header))
    assert {k: int(v) for k, v in enum.items()} == {"FTN_FILTER_BOX": 0, "FTN_FILTER_TRIANGLE": 1, "FTN_FILTER_GAUSSIAN": 2, "FTN_FILTER_MITCHELL": 3,
                                                    "FTN_FILTER_SINC": 4}


def test_defaults_of_every_kind(ftn):
    from fountain_amd.filters import Filter, KINDS
    want = {"box": (0.5, (0.0, 0.0)), "triangle": (2.0, (0.0, 0.0)), "gaussian": (2.0, (2.0, 0.0)),
            "mitchell": (2.0, (F32(1.0) / F32(3.0), F32(1.0) / F32(3.0))), "sinc": (4.0, (3.0, 0.0))}
    assert sorted(KINDS) == sorted(want) == sorted(FR.KINDS)
    for kind, (r, prm) in want.items():
        d = Filter(kind, be=ftn).desc
        assert d.kind == KINDS[kind] and tuple(d.radius) == (r, r) and tuple(d.param) == tuple(float(p) for p in prm) and tuple(d.reserved) == (0, 0, 0)
    d = A.ftn_filter_desc()
    assert ftn.lib.ftn_filter_init(5, C.byref(d)) == INV and ftn.lib.ftn_filter_init(0, None) == INV
    f = Filter("gaussian", (1.5, 0.75), be=ftn, alpha=1.25)
    assert f.radius == (1.5, 0.75) and f.desc.param[0] == 1.25
    with pytest.raises(ValueError):
        Filter("gaussian", be=ftn, tau=2.0)
    with pytest.raises(ValueError):
        Filter("lanczos", be=ftn)


TABLES = [("box", None, {}), ("box", (3.0, 0.25), {}), ("triangle", None, {}), ("triangle", (1.5, 0.75), {}), ("gaussian", None, {}),
          ("gaussian", (8.0, 0.5), dict(alpha=0.3)), ("mitchell", None, {}), ("mitchell", (4.0, 1.5), dict(B=0.0, C=0.5)), ("sinc", None, {}),
          ("sinc", (8.0, 2.0), dict(tau=2.0)), ("sinc", (0.5, 0.5), {})]


@pytest.mark.parametrize("kind,radius,params", TABLES)
def test_table_against_float64(ftn, kind, radius, params):
    """Each entry is a binary64 libm result rounded once to binary32, so it lies within 1 binary32 ulp of any other correctly working
    binary64 evaluation rounded the same way (the two may straddle a rounding boundary)."""
    from fountain_amd.filters import Filter
    f = Filter(kind, radius, be=ftn, **params)
    got = f.table()
    want = FR.table64(*FR.desc_params(f))
    assert got.shape == (16, 16) and got.dtype == F32
    w32 = want.astype(F32)
    ulp = np.maximum(np.spacing(np.abs(w32)), np.spacing(np.abs(got)))
    assert (np.abs(got.astype(np.float64) - w32.astype(np.float64)) <= ulp).all()
    if kind == "box":
        assert (got == 1.0).all()
    if kind in ("mitchell", "sinc") and radius is None:
        assert (got < 0).any() and (got > 0).any()
    if kind in ("triangle", "gaussian"):
        assert (got >= 0).all() and got[0, 0] == got.max()
    # [y][x]: with unequal radii the tables of the filters that depend on x and y themselves (not on x / rx) are not symmetric, and the
    # row index is y
    if radius is not None and radius[0] != radius[1] and kind in ("gaussian", "sinc"):
        assert not np.array_equal(got, got.T) and not (np.abs(got.astype(np.float64) - want.T.astype(F32)) <= ulp).all()


def _desc(kind=A.FTN_FILTER_GAUSSIAN, radius=(2.0, 2.0), param=(2.0, 0.0)):
    d = A.ftn_filter_desc()
    d.kind, d.radius[0], d.radius[1], d.param[0], d.param[1] = kind, radius[0], radius[1], param[0], param[1]
    return d


BAD_FILTERS = [dict(kind=5), dict(kind=0xffffffff), dict(radius=(float("nan"), 2.0)), dict(radius=(2.0, float("inf"))), dict(radius=(0.0, 2.0)),
               dict(radius=(2.0, -1.0)), dict(radius=(8.5, 2.0)), dict(radius=(2.0, np.nextafter(F32(8.0), F32(9.0)))),
               dict(param=(float("nan"), 0.0)), dict(param=(2.0, float("inf"))), dict(kind=A.FTN_FILTER_SINC, param=(0.0, 0.0)),
               dict(kind=A.FTN_FILTER_SINC, param=(-3.0, 0.0))]


def test_table_refusals(ftn):
    out = np.zeros(256, F32)
    O = out.ctypes.data_as(C.c_void_p)
    assert ftn.lib.ftn_filter_table(None, O) == INV and ftn.lib.ftn_filter_table(C.byref(_desc()), None) == INV
    for kw in BAD_FILTERS:
        assert ftn.lib.ftn_filter_table(C.byref(_desc(**kw)), O) == INV, kw
    assert not out.any()
    assert ftn.lib.ftn_filter_table(C.byref(_desc(radius=(8.0, 8.0))), O) == A.FTN_OK and out.any()


def _args(ftn, radius=(2.0, 2.0), integrator=None, sampler=None, pipeline=A.FTN_PIPELINE_AUTO):
    from fountain_amd import PathIntegrator, PerspectiveCamera, RandomSampler, Film, Transform
    cam = PerspectiveCamera(ftn, Transform.identity(ftn), (8, 8))
    film = Film(ftn, (8, 8))
    film.desc.filter_radius[0], film.desc.filter_radius[1] = radius
    smp = sampler or RandomSampler(2, 0, indexed=True)
    integ = integrator or PathIntegrator(3, 1.0)
    tr, opt, st = A.ftn_tile_range(), A.ftn_render_options(), A.ftn_stats()
    tr.stride, opt.device, opt.pipeline = 1, -1, pipeline
    keep = (cam, film, smp, integ, tr, opt)
    return [C.byref(cam.desc), C.byref(film.desc), C.byref(smp.desc), C.byref(integ.desc), C.byref(tr), C.byref(opt)], st, keep


def _render_calls(ftn, scene, args, filt, P, st):
    """both render entries with the filter in its place (behind the film)"""
    a = args[:2] + [C.byref(filt) if filt is not None else None] + args[2:]
    return (ftn.lib.ftn_render_filtered(scene, *a, P, C.byref(st)), ftn.lib.ftn_render_filtered_device(scene, *a, P, None, C.byref(st)))


def test_render_refusals_in_order(ftn):
    """null arguments; the filter's own refusals; the radius mismatch; then the moments pass's refusals (tile-serial sampler, bad sample
    range, unknown integrator, megakernel, unknown pipeline) -- each reached only when everything before it is in order, all before the
    device check, on any machine"""
    from fountain_amd import RandomSampler, PathIntegrator
    scene = C.byref((C.c_uint8 * 65536)())                   # stands in for a handle: these refusals never look at it
    px = np.zeros((8, 8, 4), F32)
    P = px.ctypes.data_as(C.c_void_p)
    args, st, keep = _args(ftn)
    good = _desc()
    assert _render_calls(ftn, None, args, good, P, st) == (INV, INV)
    assert _render_calls(ftn, scene, args, None, P, st) == (INV, INV)
    assert _render_calls(ftn, scene, args, good, None, st) == (INV, INV)
    assert _render_calls(ftn, scene, args[:1] + [None] + args[2:], good, P, st) == (INV, INV)
    # a bad filter wins over everything behind it: here the sampler is tile-serial (UNSUPPORTED) and the radius differs as well
    bad_args, st, keep2 = _args(ftn, radius=(0.5, 0.5), sampler=RandomSampler(2, 0))
    for kw in BAD_FILTERS:
        assert _render_calls(ftn, scene, bad_args, _desc(**kw), P, st) == (INV, INV), kw
    # the radius mismatch (bit for bit) wins over the sampler
    assert _render_calls(ftn, scene, bad_args, good, P, st) == (INV, INV)
    near, st, keep3 = _args(ftn, radius=(2.0, float(np.nextafter(F32(2.0), F32(3.0)))))
    assert _render_calls(ftn, scene, near, good, P, st) == (INV, INV)
    assert b"bit for bit" in ftn.fn("last_error")()
    # the moments pass's refusals, in its order
    for kw, want in ((dict(sampler=RandomSampler(2, 0)), UNS), (dict(sampler=RandomSampler(4, 0, indexed=True, first_sample=3, sample_count=2)), INV),
                     (dict(sampler=RandomSampler(4, 0, indexed=True, first_sample=5)), INV), (dict(pipeline=A.FTN_PIPELINE_MEGAKERNEL), UNS),
                     (dict(pipeline=7), INV)):
        a, st, k = _args(ftn, **kw)
        assert _render_calls(ftn, scene, a, good, P, st) == (want, want), kw
    integ = PathIntegrator(3, 1.0)
    integ.desc.kind = 9
    a, st, k = _args(ftn, integrator=integ, pipeline=A.FTN_PIPELINE_MEGAKERNEL)     # the integrator is looked at before the pipeline
    assert _render_calls(ftn, scene, a, good, P, st) == (INV, INV)
    assert b"integrator" in ftn.fn("last_error")()
    a, st, k = _args(ftn, sampler=RandomSampler(2, 0), pipeline=A.FTN_PIPELINE_MEGAKERNEL)   # ... and the sampler before both
    assert _render_calls(ftn, scene, a, good, P, st) == (UNS, UNS)
    assert b"FTN_SAMPLER_INDEXED" in ftn.fn("last_error")()
    assert not px.any()


def test_render_without_gpu_reports_no_device(ftn):
    """No CPU fallback: valid arguments and no device -> FTN_ERR_NO_DEVICE, after every refusal"""
    if ftn.fn("device_count")() > 0:
        pytest.skip("a GPU is present")
    from fountain_amd import DirectLightingIntegrator, PathIntegrator
    scene = C.byref((C.c_uint8 * 65536)())
    px = np.zeros((8, 8, 4), F32)
    P = px.ctypes.data_as(C.c_void_p)
    for integ in (PathIntegrator(3, 1.0), DirectLightingIntegrator(3)):
        for pl in (A.FTN_PIPELINE_AUTO, A.FTN_PIPELINE_WAVEFRONT):
            for kind in range(5):
                d = A.ftn_filter_desc()
                assert ftn.lib.ftn_filter_init(kind, C.byref(d)) == 0
                a, st, keep = _args(ftn, radius=tuple(d.radius), integrator=integ, pipeline=pl)
                assert _render_calls(ftn, scene, a, d, P, st) == (NODEV, NODEV)
    assert not px.any()


def test_twin_refusals_in_order(ftn):
    from fountain_amd import Film
    from fountain_amd.filters import _lib
    lib = _lib(ftn)
    film = Film(ftn, (8, 8))
    film.desc.filter_radius[0] = film.desc.filter_radius[1] = 2.0
    n = 3
    px, py, s = np.array([1, 2, 1], np.int32), np.array([1, 1, 1], np.int32), np.array([0, 0, 1], np.uint32)
    pf, L, out = np.full((n, 2), 1.5, F32), np.ones((n, 3), F32), np.zeros((8, 8, 4), F32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda film_, filt_, n_, *arr: lib.ftn_filter_accumulate_samples(film_, filt_, n_, *[ptr(a) if a is not None else None for a in arr])
    good = _desc()
    F, G = C.byref(film.desc), C.byref(good)
    assert call(None, G, n, px, py, s, pf, L, out) == INV and call(F, None, n, px, py, s, pf, L, out) == INV
    assert call(F, G, n, px, py, s, pf, L, None) == INV and call(F, G, n, px, None, s, pf, L, out) == INV
    dup = np.array([0, 0, 0], np.uint32)                                        # records 0 and 2 then share (sample, py, px)
    for kw in BAD_FILTERS:                                                       # the filter's refusals win over the radius and the duplicate
        assert call(F, C.byref(_desc(**kw)), n, px, py, dup, pf, L, out) == INV, kw
    assert call(F, C.byref(_desc(radius=(2.0, 1.5))), n, px, py, dup, pf, L, out) == INV and b"bit for bit" in ftn.fn("last_error")()
    assert call(F, G, n, px, py, dup, pf, L, out) == INV and b"share" in ftn.fn("last_error")()
    assert not out.any()
    assert call(F, G, n, px, py, s, pf, L, out) == 0 and out.any()
    assert call(F, G, 0, None, None, None, None, None, out) == 0


def test_oracle_backend_has_no_filtered_film(orc):
    from fountain_amd import FountainError
    from fountain_amd.filters import Filter
    with pytest.raises(FountainError) as e:
        Filter("gaussian", be=orc)
    assert "no oracle twin" in str(e.value)


PBRT = """LookAt 0 -3 0  0 0 0  0 0 1
Camera "perspective" "float fov" [40]
Film "image" "integer xresolution" [24] "integer yresolution" [16] "string filename" "f.exr"
Sampler "random" "integer pixelsamples" [2]
%s
WorldBegin
LightSource "point" "rgb I" [5 5 5] "point from" [0 -2 2]
Material "matte" "rgb Kd" [0.5 0.5 0.5]
Shape "sphere" "float radius" [0.7]
WorldEnd
"""


def _parsed(ftn, tmp_path, name, statement):
    from fountain_amd import PbrtScene
    p = tmp_path / name
    p.write_text(PBRT % statement)
    return PbrtScene(str(p), ftn)


def test_loader_getter(ftn, tmp_path):
    from fountain_amd import FountainError
    from fountain_amd.filters import Filter
    plain = _parsed(ftn, tmp_path, "plain.pbrt", "")
    assert Filter.from_pbrt(plain) is None
    cases = [('PixelFilter "gaussian"', "gaussian", (2.0, 2.0), (2.0, 0.0)),
             ('PixelFilter "gaussian" "float xwidth" [1.5] "float ywidth" [0.75] "float alpha" [1.25]', "gaussian", (1.5, 0.75), (1.25, 0.0)),
             ('PixelFilter "mitchell" "float B" [0.25] "float C" [0.5] "float xwidth" [3]', "mitchell", (3.0, 2.0), (0.25, 0.5)),
             ('PixelFilter "sinc" "float tau" [2]', "sinc", (4.0, 4.0), (2.0, 0.0)), ('PixelFilter "triangle" "float ywidth" [1]', "triangle", (2.0, 1.0), (0.0, 0.0)),
             ('PixelFilter "box"', "box", (0.5, 0.5), (0.0, 0.0))]
    for k, (stmt, kind, radius, param) in enumerate(cases):
        parsed = _parsed(ftn, tmp_path, "f%d.pbrt" % k, stmt)
        f = Filter.from_pbrt(parsed)
        assert (f.kind, f.radius, tuple(f.desc.param)) == (kind, radius, param), stmt
        # everything else the loader produces is what it produces without the statement, byte for byte: ftn_render still ignores it
        for name in ("camera", "_film_desc"):
            a, b = getattr(parsed, name), getattr(plain, name)
            a, b = (a.desc, b.desc) if name == "camera" else (a, b)
            assert bytes(a) == bytes(b), (stmt, name)
        assert tuple(parsed.film().desc.filter_radius) == (0.5, 0.5) and parsed.samples_per_pixel == plain.samples_per_pixel == 2
        d1, d2 = parsed.desc, plain.desc
        assert (d1.n_prims, d1.n_spheres, d1.n_lights, d1.n_materials) == (d2.n_prims, d2.n_spheres, d2.n_lights, d2.n_materials)
        assert bytes(d1.spheres[0]) == bytes(d2.spheres[0]) and bytes(d1.materials[0]) == bytes(d2.materials[0]) and bytes(d1.lights[0]) == bytes(d2.lights[0])
    with pytest.raises(FountainError) as e:
        Filter.from_pbrt(_parsed(ftn, tmp_path, "bad.pbrt", 'PixelFilter "lanczos"'))       # the file still loads: the statement is only read here
    assert e.value.code == INV and "lanczos" in str(e.value)


def test_cli_refusals(ftn, tmp_path):
    from fountain_amd import render
    scene = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")
    out = str(tmp_path / "a.exr")
    for extra in (["--gbuffer"], ["--denoise"], ["--denoise-guided"], ["--variance"], ["--adaptive", "0.1"], ["--exact-stream"], ["--gpus", "2"]):
        assert render.main([scene, "-o", out, "--pixel-filter", "gaussian"] + extra) == 2, extra
    assert render.main([scene, "-o", out, "--filter-width", "2"]) == 2
    assert render.main([scene, "-o", out, "--pixel-filter", "gaussian", "--filter-width", "2", "2", "2"]) == 2
    plain = tmp_path / "plain.pbrt"
    plain.write_text(PBRT % "")
    assert render.main([str(plain), "-o", out, "--pixel-filter", "scene"]) == 2           # the file has no PixelFilter statement
    with pytest.raises(SystemExit):
        render.main([scene, "-o", out, "--pixel-filter", "lanczos"])
    assert not [p for p in tmp_path.iterdir() if p.suffix == ".exr"]
