"""Per-pixel second moments and variance estimates (include/fountain_hip_moments.h): the beauty of ftn_render, bit for bit, and beside it
the sums of the squares of every camera sample's radiance, from which the variance of each pixel's mean follows.

  render_moments(be, builder, cam, res, integrator, sampler)   host buffers -> (variance [H, W, 4], film, moments [H, W, 4], stats)
  render_moments_torch(scene, cam, film, integrator, sampler, pixels, moments)   adds into float32 CUDA tensors [H, W, 4] on the current stream
  resolve(be, pixels, moments) / resolve_torch(be, pixels, moments, out)         sums -> variance of the mean, r, g, b, Y per pixel

The moments layout is ftn_moment_pixel: sq r, g, b (raw RGB radiance squared), sq_y (Y squared).  The resolved variance is +inf where the
pixel's filter weight is below 2.  The reference keeps no second moments, so the CPU oracle has no twin of these calls.
"""
import ctypes as C

import numpy as np

from . import _abi as A
from ._nontwin import bind, call_args as _call_args, check_array as _check_array, check_tensor as _check_tensor, current_stream, ptr, tptr
from .api import Film

CHANNELS = ("r", "g", "b", "Y")          # the 4 floats per pixel of the moments and of the resolved variance


def _lib(be):
    return bind(be, A.EXTENSIONS["moments"])


def resolve(be, pixels, moments):
    """ftn_moments_resolve: beauty [..., 4] (ftn_pixel) and moments [..., 4] -> variance of the mean [..., 4] (r, g, b, Y)."""
    lib = _lib(be)
    pixels = np.ascontiguousarray(pixels, dtype=np.float32)
    moments = np.ascontiguousarray(moments, dtype=np.float32)
    if pixels.shape != moments.shape or pixels.shape[-1] != 4:
        raise ValueError("pixels and moments must have the same shape [..., 4]")
    out = np.empty(pixels.shape, np.float32)
    be.check(lib.ftn_moments_resolve(ptr(pixels), ptr(moments), pixels.size // 4, ptr(out)))
    return out


def render_moments(be, builder, cam, res, integrator, sampler, tiles=None, crop=(0.0, 0.0, 1.0, 1.0), scene=None, film=None, moments=None,
                   pipeline=A.FTN_PIPELINE_AUTO, device=-1, count_traffic=False):
    """Shaped like scenes.render: create_scene (unless `scene` is given) + Film (unless `film` is given) + ftn_render_moments.  The
    beauty is added into film.pixels, the moments into `moments` ([H, W, 4] float32; a zero buffer when not given).  Returns (variance of
    the mean [H, W, 4], film, moments, stats)."""
    lib = _lib(be)
    scene = scene or builder.create_scene()
    film = film or Film(be, res, crop)
    shape = (film.height, film.width, 4)
    if moments is None:
        moments = np.zeros(shape, np.float32)
    _check_array(moments, shape, "moments")
    _check_array(film.pixels, shape, "film.pixels")
    args, keep = _call_args(cam, film, integrator, sampler, tiles, pipeline, device, count_traffic)
    st = A.ftn_stats()
    be.check(lib.ftn_render_moments(scene.handle, *args, ptr(film.pixels), ptr(moments), C.byref(st)))
    return resolve(be, film.pixels, moments), film, moments, st.as_dict()


def render_moments_torch(scene, cam, film, integrator, sampler, pixels, moments, tiles=None, pipeline=A.FTN_PIPELINE_AUTO):
    """ftn_render_moments_device into `pixels` (ftn_pixel) and `moments` (float32 CUDA tensors [H, W, 4], both added into) on the
    current stream of their device."""
    be = scene.be
    lib = _lib(be)
    shape = (film.height, film.width, 4)
    _check_tensor(pixels, shape)
    _check_tensor(moments, shape)
    if pixels.device != moments.device:
        raise ValueError("pixels and moments must be on the same device")
    args, keep = _call_args(cam, film, integrator, sampler, tiles, pipeline, pixels.device.index)
    st = A.ftn_stats()
    be.check(lib.ftn_render_moments_device(scene.handle, *args, tptr(pixels), tptr(moments),
                                           C.c_void_p(current_stream(pixels)), C.byref(st)))
    return st.as_dict()


def resolve_torch(be, pixels, moments, out):
    """ftn_moments_resolve_device: pixels, moments -> out, float32 CUDA tensors [..., 4], on the current stream."""
    lib = _lib(be)
    for t in (pixels, moments, out):
        _check_tensor(t, pixels.shape)
    if pixels.shape[-1] != 4:
        raise ValueError("the last dimension holds the 4 floats of a pixel")
    be.check(lib.ftn_moments_resolve_device(tptr(pixels), tptr(moments), pixels.numel() // 4,
                                            tptr(out), C.c_void_p(current_stream(pixels))))
    return out
