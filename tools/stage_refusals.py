"""The refusals of the image-space stages' C entry points, as a transcript: for every entry of include/fountain_hip_{denoise,
denoise_guided,temporal,display,bloom}.h a fixed list of bad calls -- each pointer null in turn, w = 0, w * h = 2^31, each params field
out of range, and for the device entries each overlapping pair of buffers and each buffer misaligned -- and one good call, which on a
machine without a GPU is the no-device refusal of every entry but the host twins.  Then the render and resolve entries of the passes
beside the beauty (include/fountain_hip_{gbuffer,idmatte,moments}.h): each pointer null in turn, the tile-serial and an unknown sampler,
the megakernel and an unknown pipeline, a filter radius above 1, a sample range outside, pairs of those (which one an entry reports
first), and the good call.  Prints `entry, case, status, ftn_last_error()`.

  python tools/stage_refusals.py [path/to/libfountain_hip.so] > transcript.txt

Needs no device (run it where there is none: the good calls of the device entries are given host memory).  Two builds that refuse alike
print the same bytes; profiles/stage_host/ keeps such a comparison.
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fountain_amd import _abi as A  # noqa: E402

W, H = 4, 3
NAN, INF = float("nan"), float("inf")
HIST_BYTES = 4 * A.FTN_DISPLAY_HIST_WORDS

# out-of-range values per params struct: (field, value), applied to the defaults one at a time
BAD_FIELDS = {
    "ftn_denoise_params": [("levels", -1), ("levels", 11), ("flags", 2), ("reserved", 1)]
    + [(f, v) for f in ("sigma_color", "sigma_normal", "sigma_plane") for v in (0.0, -1.0, NAN, INF)]
    + [(f, v) for f in ("albedo_eps", "color_eps") for v in (-1.0, NAN, INF)],
    "ftn_denoise_guided_params": [("levels", -1), ("levels", 11), ("flags", 2), ("reserved", 1)]
    + [(f, v) for f in ("sigma_variance", "sigma_normal", "sigma_plane") for v in (0.0, -1.0, NAN, INF)]
    + [(f, v) for f in ("albedo_eps", "rel_eps") for v in (-1.0, NAN, INF)],
    "ftn_temporal_params": [("flags", 2), ("reserved", (0, 1)), ("reserved", (1, 0))]
    + [("alpha_min", v) for v in (-0.01, 1.01, NAN, INF)]
    + [(f, v) for f in ("normal_tol", "plane_tol", "albedo_tol", "albedo_eps") for v in (-1e-3, NAN, INF)],
    "ftn_display_params": [("tonemap", 4), ("transfer", 3), ("flags", 4), ("reserved", 1)]
    + [(f, v) for f in ("ev", "key", "white", "gamma") for v in (NAN, INF)]
    + [(f, v) for f in ("key", "white", "gamma") for v in (0.0, -1.0)]
    + [("p_lo", -0.1), ("p_lo", 0.96), ("p_hi", 1.1), ("p_lo", NAN), ("min_ev", 17.0), ("max_ev", NAN)],
    "ftn_bloom_params": [("levels", -1), ("levels", 13), ("flags", 2), ("reserved", 1)]
    + [(f, v) for f in ("strength", "scatter", "threshold", "knee", "clamp_max") for v in (NAN, INF, -0.5)]
    + [(f, 1.5) for f in ("strength", "scatter", "knee")] + [("clamp_max", 0.0), ("clamp_max", 2e30)],
}


def buf(name, per_pixel=0, fixed=0):
    return ("buf", name, per_pixel, fixed)


IMG = [buf("rgb", 12), ("w",), ("h",)]
DN = [buf("rgb", 12), buf("gb12", 48)]
TP = [buf("rgb", 12), buf("gb12", 48), buf("var4", 16), ("ref", "cur_camera", "camera"), ("ref", "film", "film"), ("w",), ("h",),
      ("ref", "prev_camera", "camera"), buf("prev_gb12", 48), buf("prev_history", 32), ("params", "ftn_temporal_params"), buf("out_history", 32),
      buf("out_rgb", 12), buf("out_var4", 16)]
DEVICE, STREAM = ("val", C.c_int32(-1)), ("val", C.c_void_p(None))
ENTRIES = [
    ("ftn_denoise_workspace_size", [("w",), ("h",), ("ref", "bytes", "size_t")]),
    ("ftn_denoise_device", DN + [("w",), ("h",), ("params", "ftn_denoise_params"), buf("out_rgb", 12), buf("workspace", 64), STREAM]),
    ("ftn_denoise", DN + [("w",), ("h",), ("params", "ftn_denoise_params"), buf("out_rgb", 12), DEVICE]),
    ("ftn_denoise_cpu", DN + [("w",), ("h",), ("params", "ftn_denoise_params"), buf("out_rgb", 12)]),
    ("ftn_denoise_guided_workspace_size", [("w",), ("h",), ("ref", "bytes", "size_t")]),
    ("ftn_denoise_guided_device", DN + [buf("var4", 16), ("w",), ("h",), ("params", "ftn_denoise_guided_params"), buf("out_rgb", 12), buf("workspace", 64),
                                        STREAM]),
    ("ftn_denoise_guided", DN + [buf("var4", 16), ("w",), ("h",), ("params", "ftn_denoise_guided_params"), buf("out_rgb", 12), DEVICE]),
    ("ftn_denoise_guided_cpu", DN + [buf("var4", 16), ("w",), ("h",), ("params", "ftn_denoise_guided_params"), buf("out_rgb", 12)]),
    ("ftn_temporal_accumulate_device", TP + [STREAM]),
    ("ftn_temporal_accumulate", TP + [DEVICE]),
    ("ftn_temporal_accumulate_cpu", TP),
    ("ftn_display_histogram_device", IMG + [buf("hist", fixed=HIST_BYTES), STREAM]),
    ("ftn_display_histogram", IMG + [buf("hist", fixed=HIST_BYTES), DEVICE]),
    ("ftn_display_histogram_cpu", IMG + [buf("hist", fixed=HIST_BYTES)]),
    ("ftn_display_exposure", [buf("hist", fixed=HIST_BYTES), ("params", "ftn_display_params"), ("ref", "info", "info")]),
    ("ftn_display_encode_device", IMG + [("params", "ftn_display_params"), ("scale",), buf("out_rgb", 12), buf("out_rgba8", 4), STREAM]),
    ("ftn_display_encode", IMG + [("params", "ftn_display_params"), ("scale",), buf("out_rgb", 12), buf("out_rgba8", 4), DEVICE]),
    ("ftn_display_encode_cpu", IMG + [("params", "ftn_display_params"), ("scale",), buf("out_rgb", 12), buf("out_rgba8", 4)]),
    ("ftn_display", IMG + [("params", "ftn_display_params"), buf("out_rgb", 12), buf("out_rgba8", 4), ("ref", "info", "info"), DEVICE]),
    ("ftn_bloom_workspace_size", [("w",), ("h",), ("levels",), ("ref", "bytes", "size_t")]),
    ("ftn_bloom_device", IMG + [("params", "ftn_bloom_params"), buf("out_rgb", 12), buf("workspace", 64), STREAM]),
    ("ftn_bloom", IMG + [("params", "ftn_bloom_params"), buf("out_rgb", 12), DEVICE]),
    ("ftn_bloom_cpu", IMG + [("params", "ftn_bloom_params"), buf("out_rgb", 12)]),
]


def camera():
    """a pinhole at the origin looking down +z, focal length 2 pixels (matrices column-major)"""
    d = A.ftn_camera_desc()
    eye = [1.0 if i % 5 == 0 else 0.0 for i in range(16)]
    c2r = [[2.0, 0, W / 2.0, 0], [0, 2.0, H / 2.0, 0], [0, 0, 1, -0.01], [0, 0, 1, 0]]
    r2c = [[0.5, 0, 0, -W / 4.0], [0, 0.5, 0, -H / 4.0], [0, 0, 0, 1], [0, 0, -100.0, 100.0]]
    flat = lambda m: (C.c_float * 16)(*[m[r][c] for c in range(4) for r in range(4)])
    d.camera_to_world.m, d.camera_to_world.inv = (C.c_float * 16)(*eye), (C.c_float * 16)(*eye)
    d.raster_to_camera.m, d.raster_to_camera.inv = flat(r2c), flat(c2r)
    d.shutter_open, d.shutter_close, d.lens_radius, d.focal_dist = 0.0, 1.0, 0.0, 1e6
    return d


def film():
    d = A.ftn_film_desc()
    d.full_resolution, d.crop, d.filter_radius = (C.c_int32 * 2)(W, H), (C.c_int32 * 4)(0, 0, W, H), (C.c_float * 2)(0.5, 0.5)
    return d


class Call:
    """One entry's good arguments (a 4 x 3 image; every buffer 64-byte aligned, filled with 0.5, with room to be moved by 8 bytes)."""

    def __init__(self, lib, name, spec):
        self.fn, self.spec, self.keep, self.args, self.ranges = getattr(lib, name), spec, [], [], {}
        self.fn.restype, self.fn.argtypes = C.c_int, None
        for i, a in enumerate(spec):
            if a[0] == "buf":
                n = a[2] * W * H + a[3]
                raw = (C.c_float * (n // 4 + 64))(*([0.5] * (n // 4 + 64)))
                at = (C.addressof(raw) + 63) // 64 * 64
                self.keep.append(raw)
                self.ranges[i] = (at, n)
                self.args.append(C.c_void_p(at))
            elif a[0] == "params":
                p = getattr(A, a[1])()
                getattr(lib, a[1] + "_default")(C.byref(p))
                self.args.append(p)
            elif a[0] == "ref":
                self.args.append({"camera": camera, "film": film, "size_t": C.c_size_t, "info": A.ftn_display_info}[a[2]]())
            else:
                self.args.append({"w": C.c_int32(W), "h": C.c_int32(H), "levels": C.c_int32(6), "scale": C.c_float(1.0)}.get(a[0]) or a[1])

    def run(self, **replace):
        """the status and message of the call with arguments replaced by position"""
        args = [replace.get("a%d" % i, v) for i, v in enumerate(self.args)]
        args = [C.byref(v) if isinstance(v, C.Structure) or isinstance(v, C.c_size_t) else v for v in args]
        return self.fn(*args)


def cases(call):
    spec = call.spec
    yield "good", {}
    for i, a in enumerate(spec):
        if a[0] in ("buf", "params", "ref"):
            yield "null %s" % a[1], {"a%d" % i: None}
    names = [a[0] for a in spec]
    if "w" in names:
        yield "w = 0", {"a%d" % names.index("w"): C.c_int32(0)}
        yield "w * h = 2^31", {"a%d" % names.index("w"): C.c_int32(65536), "a%d" % names.index("h"): C.c_int32(32768)}
    if "levels" in names:
        for v in (-1, 13):
            yield "levels = %d" % v, {"a%d" % names.index("levels"): C.c_int32(v)}
    if "scale" in names:
        for v in (-1.0, NAN, INF):
            yield "scale = %r" % v, {"a%d" % names.index("scale"): C.c_float(v)}
    if "params" in names:
        i = names.index("params")
        for field, v in BAD_FIELDS[spec[i][1]]:
            p = type(call.args[i])()
            C.memmove(C.byref(p), C.byref(call.args[i]), C.sizeof(p))
            if isinstance(v, tuple):
                p.reserved[v[0]] = 1
            else:
                setattr(p, field, v)
            yield "%s = %r" % (field, v), {"a%d" % i: p}
    if call.fn.__name__.endswith("_device"):
        bufs = sorted(call.ranges)
        for n, i in enumerate(bufs):
            for j in bufs[n + 1:]:
                # the second buffer moved onto the first one's last 16 bytes (both stay 16-byte aligned)
                yield "%s overlaps %s" % (spec[j][1], spec[i][1]), {"a%d" % j: C.c_void_p(call.ranges[i][0] + call.ranges[i][1] // 16 * 16 - 16)}
        for i in bufs:
            for by in (2, 8):
                yield "%s + %d bytes" % (spec[i][1], by), {"a%d" % i: C.c_void_p(call.ranges[i][0] + by)}
    if "prev_history" in [a[1] for a in spec if len(a) > 1]:
        prev = [i for i, a in enumerate(spec) if len(a) > 1 and str(a[1]).startswith("prev_")]
        yield "first frame", {"a%d" % i: None for i in prev}
    if call.fn.__name__ == "ftn_display_exposure":
        p = type(call.args[1])()
        C.memmove(C.byref(p), C.byref(call.args[1]), C.sizeof(p))
        p.flags = A.FTN_DISPLAY_AUTO_EXPOSURE
        yield "null hist, automatic", {"a0": None, "a1": p}


# ---------------------------------------------------------------------- the render passes beside the beauty
# The render and resolve entries of include/fountain_hip_{gbuffer,idmatte,moments}.h.  Arguments by name, in call order; "scene" is 64 KiB
# of zeros (no entry looks behind the handle before it has found a device), the pixel buffers are host memory.
PASS_RENDER = {
    "gbuffer": ["scene", "cam", "film", "sd", "tr", "opt", "pixels"],
    "idmatte": ["scene", "cam", "film", "sd", "tr", "opt", "prim_ids", "n_prim_ids", "pixels"],
    "moments": ["scene", "cam", "film", "sd", "id", "tr", "opt", "pixels", "moments"],
}
PASS_RESOLVE = {"gbuffer": ["in", "n", "out"], "idmatte": ["in", "n", "out"], "moments": ["beauty", "in", "n", "out"]}
PASS_OPTIONAL = ("tr", "opt", "stream", "st")          # null is a good value


def pass_args(names):
    sd = A.ftn_sampler_desc(A.FTN_SAMPLER_INDEXED, 4, 7, 1, 2)
    made = {"scene": (C.c_char * 65536)(), "cam": camera(), "film": film(), "sd": sd, "id": A.ftn_integrator_desc(A.FTN_INTEGRATOR_PATH, 5, 1.0, 0),
            "tr": None, "opt": None, "stream": C.c_void_p(None), "st": None, "prim_ids": (C.c_uint32 * 4)(1, 2, 3, 4), "n_prim_ids": C.c_size_t(4),
            "n": C.c_size_t(W * H)}
    for k in ("pixels", "moments", "in", "out", "beauty"):
        made[k] = (C.c_float * (20 * W * H))()
    return [made[k] for k in names]


def pass_cases(names, render):
    yield "good", {}
    for k in names:
        if k not in PASS_OPTIONAL and not k.startswith("n"):
            yield "null %s" % k, {k: None}
    if not render:
        yield "n = 0, all null", {k: (C.c_size_t(0) if k == "n" else None) for k in names if k != "stream"}
        return
    for label, kind in (("tile-serial sampler", A.FTN_SAMPLER_TILE_SERIAL), ("unknown sampler", 7)):
        yield label, {"sd": A.ftn_sampler_desc(kind, 4, 7, 1, 2)}
    for label, pl in (("megakernel pipeline", A.FTN_PIPELINE_MEGAKERNEL), ("unknown pipeline", 9)):
        yield label, {"opt": A.ftn_render_options(pl, -1, 0, 0)}
    f = film()
    f.filter_radius[1] = 1.5
    yield "filter radius 1.5", {"film": f}
    yield "first_sample beyond samples_per_pixel", {"sd": A.ftn_sampler_desc(A.FTN_SAMPLER_INDEXED, 4, 7, 5, 0)}
    yield "sample range beyond samples_per_pixel", {"sd": A.ftn_sampler_desc(A.FTN_SAMPLER_INDEXED, 4, 7, 3, 2)}
    # two refusals at once: the first in the entry's order is the one reported
    yield "tile-serial sampler, megakernel pipeline", {"sd": A.ftn_sampler_desc(A.FTN_SAMPLER_TILE_SERIAL, 4, 7, 1, 2), "opt": A.ftn_render_options(A.FTN_PIPELINE_MEGAKERNEL, -1, 0, 0)}
    yield "megakernel pipeline, sample range outside", {"sd": A.ftn_sampler_desc(A.FTN_SAMPLER_INDEXED, 4, 7, 3, 2), "opt": A.ftn_render_options(A.FTN_PIPELINE_MEGAKERNEL, -1, 0, 0)}
    yield "filter radius 1.5, sample range outside", {"film": f, "sd": A.ftn_sampler_desc(A.FTN_SAMPLER_INDEXED, 4, 7, 3, 2)}
    if "id" in names:
        yield "unknown integrator, unknown pipeline", {"id": A.ftn_integrator_desc(9, 5, 1.0, 0), "opt": A.ftn_render_options(9, -1, 0, 0)}
        yield "sample range outside, max_depth 65536", {"sd": A.ftn_sampler_desc(A.FTN_SAMPLER_INDEXED, 4, 7, 3, 2), "id": A.ftn_integrator_desc(A.FTN_INTEGRATOR_PATH, 65536, 1.0, 0)}


def pass_entries(lib):
    """(entry, argument names, is it a render entry) of the three headers"""
    for p in ("gbuffer", "idmatte", "moments"):
        yield "ftn_render_%s_device" % p, PASS_RENDER[p] + ["stream", "st"], True
        yield "ftn_render_%s" % p, PASS_RENDER[p] + ["st"], True
        yield "ftn_%s_resolve" % p, PASS_RESOLVE[p], False
        yield "ftn_%s_resolve_device" % p, PASS_RESOLVE[p] + ["stream"], False


def run_passes(lib):
    if lib.ftn_device_count() > 0:          # a call that gets as far as the device would look behind the scene handle
        print("the render passes' entries: left out, a device is present")
        return
    for name, names, render in pass_entries(lib):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = C.c_int, None
        good = pass_args(names)
        for case, replace in pass_cases(names, render):
            args = [replace.get(k, v) for k, v in zip(names, good)]
            args = [C.byref(v) if isinstance(v, C.Structure) else v for v in args]
            status = fn(*args)
            print("%s, %s, %d, %s" % (name, case, status, lib.ftn_last_error().decode() if status else ""))


def main(argv):
    path = argv[1] if len(argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fountain_amd", "libfountain_hip.so")
    lib = C.CDLL(path)
    lib.ftn_last_error.restype = C.c_char_p
    for name, spec in ENTRIES:
        call = Call(lib, name, spec)
        for case, replace in cases(call):
            status = call.run(**replace)
            print("%s, %s, %d, %s" % (name, case, status, lib.ftn_last_error().decode() if status else ""))
    run_passes(lib)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
