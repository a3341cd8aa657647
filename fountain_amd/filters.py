"""Reconstruction-filtered films (include/fountain_hip_filter.h): box, triangle, Gaussian, Mitchell and Lanczos-sinc filters with
PBRT v3's definitions, rendered by a deterministic gather beside ftn_render's passes.

  Filter(kind, radius=None, be=None, **params)   kind: "box" | "triangle" | "gaussian" | "mitchell" | "sinc"; radius: r or (rx, ry);
                                            params: alpha (gaussian), B, C (mitchell), tau (sinc); .table() -> [16, 16] float32
  Filter.from_pbrt(parsed)                  the PixelFilter statement of a PbrtScene, or None
  render_filtered(be, builder, cam, res, integrator, sampler, filt)       host buffers -> (rgb [H, W, 3], film, stats)
  render_filtered_torch(scene, cam, film, integrator, sampler, filt, pixels)   adds into a float32 CUDA tensor [H, W, 4] on the current stream
  accumulate_samples(be, film, filt, px, py, sample, p_film, L, out=None) the host twin: the same film from a list of camera samples

The film's filter_radius must be the filter's: filtered_film() makes such a film.  The reference's only filter is the box, so the CPU
oracle has no twin of these calls.
"""
import ctypes as C

import numpy as np

from . import _abi as A
from ._nontwin import bind, call_args as _call_args, check_array as _check_array, check_tensor as _check_tensor, current_stream, ptr, tptr
from .api import Film, FountainError, default_backend

KINDS = {"box": A.FTN_FILTER_BOX, "triangle": A.FTN_FILTER_TRIANGLE, "gaussian": A.FTN_FILTER_GAUSSIAN, "mitchell": A.FTN_FILTER_MITCHELL,
         "sinc": A.FTN_FILTER_SINC}
PARAMS = {"box": (), "triangle": (), "gaussian": ("alpha",), "mitchell": ("B", "C"), "sinc": ("tau",)}


def _lib(be):
    return bind(be, A.EXTENSIONS["filter"])


class Filter:
    def __init__(self, kind, radius=None, be=None, **params):
        """ftn_filter_init's defaults of `kind`, then the radius (one number or (rx, ry)) and the kind's parameters where given; `be`:
        the backend (the default one when not given)."""
        be = be or default_backend()
        if kind not in KINDS:
            raise ValueError("unknown filter %r: one of %s" % (kind, ", ".join(KINDS)))
        unknown = set(params) - set(PARAMS[kind])
        if unknown:
            raise ValueError("the %s filter has no parameter %s" % (kind, ", ".join(sorted(unknown))))
        self.be, self.kind = be, kind
        self.desc = A.ftn_filter_desc()
        be.check(_lib(be).ftn_filter_init(KINDS[kind], C.byref(self.desc)))
        if radius is not None:
            rx, ry = (radius, radius) if np.isscalar(radius) else radius
            self.desc.radius[0], self.desc.radius[1] = rx, ry
        for k, name in enumerate(PARAMS[kind]):
            if name in params:
                self.desc.param[k] = params[name]

    @classmethod
    def from_desc(cls, be, desc):
        f = cls.__new__(cls)
        f.be, f.kind = be, [k for k, v in KINDS.items() if v == desc.kind][0]
        f.desc = A.ftn_filter_desc()
        C.memmove(C.byref(f.desc), C.byref(desc), C.sizeof(desc))
        return f

    @classmethod
    def from_pbrt(cls, parsed):
        """ftn_pbrt_filter: the PixelFilter statement of a parsed scene file, or None when it has none."""
        desc = A.ftn_filter_desc()
        rc = _lib(parsed.be).ftn_pbrt_filter(parsed.handle, C.byref(desc))
        if rc < 0:
            raise FountainError(rc, parsed.be.lib.ftn_pbrt_last_error().decode(errors="replace"))
        return cls.from_desc(parsed.be, desc) if rc else None

    @property
    def radius(self):
        return (float(self.desc.radius[0]), float(self.desc.radius[1]))

    def table(self):
        """ftn_filter_table: Film::new's 16 x 16 table, [y, x]."""
        out = np.empty((16, 16), np.float32)
        self.be.check(_lib(self.be).ftn_filter_table(C.byref(self.desc), ptr(out)))
        return out


def filtered_film(be, filt, res=None, crop=(0.0, 0.0, 1.0, 1.0), film=None):
    """A Film of resolution `res` (or a copy of `film`'s description with fresh pixels) whose filter_radius is the filter's."""
    f = Film.from_desc(be, film.desc) if film is not None else Film(be, res, crop)
    f.desc.filter_radius[0], f.desc.filter_radius[1] = filt.desc.radius[0], filt.desc.radius[1]
    return f


def render_filtered(be, builder, cam, res, integrator, sampler, filt, tiles=None, crop=(0.0, 0.0, 1.0, 1.0), scene=None, film=None,
                    pipeline=A.FTN_PIPELINE_AUTO, device=-1, count_traffic=False):
    """Shaped like moments.render_moments: create_scene (unless `scene` is given) + a film with the filter's radius (unless `film` is
    given) + ftn_render_filtered, added into film.pixels.  Returns (resolved rgb [H, W, 3], film, stats)."""
    lib = _lib(be)
    scene = scene or builder.create_scene()
    film = film or filtered_film(be, filt, res, crop)
    _check_array(film.pixels, (film.height, film.width, 4), "film.pixels")
    args, keep = _call_args(cam, film, integrator, sampler, tiles, pipeline, device, count_traffic)
    st = A.ftn_stats()
    be.check(lib.ftn_render_filtered(scene.handle, args[0], args[1], C.byref(filt.desc), *args[2:], ptr(film.pixels), C.byref(st)))
    return film.into_spectrum_buffer()[0], film, st.as_dict()


def render_filtered_torch(scene, cam, film, integrator, sampler, filt, pixels, tiles=None, pipeline=A.FTN_PIPELINE_AUTO):
    """ftn_render_filtered_device into `pixels` (ftn_pixel: a float32 CUDA tensor [H, W, 4], added into) on the current stream of its
    device."""
    be = scene.be
    lib = _lib(be)
    _check_tensor(pixels, (film.height, film.width, 4))
    args, keep = _call_args(cam, film, integrator, sampler, tiles, pipeline, pixels.device.index)
    st = A.ftn_stats()
    be.check(lib.ftn_render_filtered_device(scene.handle, args[0], args[1], C.byref(filt.desc), *args[2:], tptr(pixels),
                                            C.c_void_p(current_stream(pixels)), C.byref(st)))
    return st.as_dict()


def accumulate_samples(be, film, filt, px, py, sample, p_film, L, out=None):
    """ftn_filter_accumulate_samples: the filtered film of n camera samples (source pixel px, py [n], sample index [n], p_film [n, 2],
    radiance L [n, 3], in any order), added into `out` ([H, W, 4] float32 ftn_pixel; a zero buffer when not given).  Returns out."""
    lib = _lib(be)
    px, py = np.ascontiguousarray(px, np.int32), np.ascontiguousarray(py, np.int32)
    sample = np.ascontiguousarray(sample, np.uint32)
    p_film, L = np.ascontiguousarray(p_film, np.float32), np.ascontiguousarray(L, np.float32)
    n = len(px)
    if py.shape != (n,) or sample.shape != (n,) or p_film.shape != (n, 2) or L.shape != (n, 3):
        raise ValueError("px, py, sample [n], p_film [n, 2] and L [n, 3] must describe the same n samples")
    shape = (film.height, film.width, 4)
    if out is None:
        out = np.zeros(shape, np.float32)
    _check_array(out, shape, "out")
    be.check(lib.ftn_filter_accumulate_samples(C.byref(film.desc), C.byref(filt.desc), n, *map(ptr, (px, py, sample, p_film, L, out))))
    return out
