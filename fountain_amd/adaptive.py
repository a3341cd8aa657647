"""Per-tile adaptive sampling (include/fountain_hip_adaptive.h): every 16x16 tile gets min_samples samples, then more, round by round, until
the estimated relative standard error of each of its pixels' mean luminance is below the threshold or it has samples_per_pixel.  A tile that
ends at n samples holds the bits of a uniform moments render (fountain_amd/moments.py) over the sample range [0, n).

  params(**overrides)                                                         ftn_adaptive_params: the library's defaults, with overrides
  render_adaptive(be, builder, cam, res, integrator, sampler, params)         host buffers -> (film, moments [H, W, 4], counts [H, W], info, stats)
  render_adaptive_torch(scene, cam, film, integrator, sampler, params, pixels, moments, counts, stream=None)   device tensors
  converged(be, pixels, moments, params)                                      the criterion per pixel, on the host (uint8 [...])

The counts are one uint32 per crop pixel, the final sample count of the pixel's tile; they are written for the tile range's pixels only.
"""
import ctypes as C

import numpy as np

from . import _abi as A
from ._nontwin import bind, call_args as _call_args, check_array as _check_array, check_tensor as _check_tensor, ptr, set_fields, tptr
from .api import Film


def _lib(be):
    return bind(be, A.EXTENSIONS["adaptive"])


def params(be, **overrides):
    """ftn_adaptive_params_default, then the given fields (min_samples, step_samples, threshold, abs_floor)."""
    p = A.ftn_adaptive_params()
    _lib(be).ftn_adaptive_params_default(C.byref(p))
    return set_fields(p, overrides)


def converged(be, pixels, moments, prm):
    """ftn_adaptive_converged: beauty [..., 4] (ftn_pixel) and moments [..., 4] -> uint8 [...], 1 where the pixel has converged."""
    lib = _lib(be)
    pixels = np.ascontiguousarray(pixels, dtype=np.float32)
    moments = np.ascontiguousarray(moments, dtype=np.float32)
    if pixels.shape != moments.shape or pixels.shape[-1] != 4:
        raise ValueError("pixels and moments must have the same shape [..., 4]")
    out = np.zeros(pixels.shape[:-1], np.uint8)
    be.check(lib.ftn_adaptive_converged(ptr(pixels), ptr(moments), pixels.size // 4, C.byref(prm), ptr(out)))
    return out


def render_adaptive(be, builder, cam, res, integrator, sampler, prm=None, tiles=None, crop=(0.0, 0.0, 1.0, 1.0), scene=None, film=None,
                    moments=None, counts=None, pipeline=A.FTN_PIPELINE_AUTO, device=-1, count_traffic=False):
    """Shaped like moments.render_moments: create_scene (unless `scene` is given) + Film (unless `film` is given) + ftn_render_adaptive.
    The beauty is added into film.pixels, the moments into `moments` ([H, W, 4] float32, zeros when not given); the counts are written
    into `counts` ([H, W] uint32, zeros when not given) for the tile range's pixels.  Returns (film, moments, counts, info, stats)."""
    lib = _lib(be)
    prm = prm if prm is not None else params(be)
    scene = scene or builder.create_scene()
    film = film or Film(be, res, crop)
    shape = (film.height, film.width, 4)
    if moments is None:
        moments = np.zeros(shape, np.float32)
    if counts is None:
        counts = np.zeros(shape[:2], np.uint32)
    _check_array(moments, shape, "moments")
    _check_array(film.pixels, shape, "film.pixels")
    if counts.shape != shape[:2] or counts.dtype != np.uint32 or not counts.flags.c_contiguous:
        raise ValueError("counts must be a C-contiguous uint32 array of shape %r" % (shape[:2],))
    args, keep = _call_args(cam, film, integrator, sampler, tiles, pipeline, device, count_traffic)
    st, info = A.ftn_stats(), A.ftn_adaptive_info()
    be.check(lib.ftn_render_adaptive(scene.handle, *args, C.byref(prm), ptr(film.pixels), ptr(moments), ptr(counts), C.byref(info), C.byref(st)))
    return film, moments, counts, info.as_dict(), st.as_dict()


def render_adaptive_torch(scene, cam, film, integrator, sampler, prm, pixels, moments, counts, tiles=None, pipeline=A.FTN_PIPELINE_AUTO, stream=None):
    """ftn_render_adaptive_device into `pixels` (ftn_pixel) and `moments` (float32 CUDA tensors [H, W, 4], both added into) and `counts`
    (an int32 CUDA tensor [H, W], holding the uint32 counts, written for the tile range's pixels), on `stream` (a torch.cuda.Stream; the
    current stream of their device when None).  The call waits for the device after every round.  Returns (info, stats)."""
    import torch
    be = scene.be
    lib = _lib(be)
    prm = prm if prm is not None else params(be)
    shape = (film.height, film.width, 4)
    _check_tensor(pixels, shape)
    _check_tensor(moments, shape)
    if (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or not counts.is_cuda or not counts.is_contiguous()
            or tuple(counts.shape) != shape[:2]):
        raise ValueError("counts must be a contiguous int32 CUDA tensor of shape %r" % (shape[:2],))
    if pixels.device != moments.device or pixels.device != counts.device:
        raise ValueError("pixels, moments and counts must be on the same device")
    args, keep = _call_args(cam, film, integrator, sampler, tiles, pipeline, pixels.device.index)
    st, info = A.ftn_stats(), A.ftn_adaptive_info()
    s = (stream or torch.cuda.current_stream(pixels.device)).cuda_stream
    be.check(lib.ftn_render_adaptive_device(scene.handle, *args, C.byref(prm), tptr(pixels), tptr(moments),
                                            tptr(counts), C.c_void_p(s), C.byref(info), C.byref(st)))
    return info.as_dict(), st.as_dict()
