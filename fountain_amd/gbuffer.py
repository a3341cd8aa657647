"""First-hit G-buffers (include/fountain_hip_gbuffer.h): albedo, shading normal, position and camera-space depth over exactly the
camera samples ftn_render traces for the same sampler, tiles and film, so that a denoiser's feature buffers line up with the beauty.

  render_gbuffer(be, builder, cam, res, sampler)   host buffers -> (resolved dict of [H, W, k] arrays, raw [H, W, 12] sums, stats)
  render_gbuffer_torch(scene, cam, film, sampler, out)   adds into a float32 CUDA tensor [H, W, 12] on the current stream
  resolve(be, raw) / resolve_torch(be, raw, out)         sums -> the 12 resolved floats per pixel

The raw layout is ftn_gbuffer_pixel: albedo 3, normal 3, position 3, depth, hit_weight, weight.  The reference renders no G-buffer, so
the CPU oracle has no twin of these calls.
"""
import ctypes as C

import numpy as np

from . import _abi as A
from ._nontwin import call_args, check_tensor as _check_tensor, checked_lib
from .api import Film

# resolved channels: name -> slice of the 12 floats ftn_gbuffer_resolve writes per pixel
CHANNELS = {"albedo": slice(0, 3), "normal": slice(3, 6), "position": slice(6, 9), "depth": slice(9, 10),
            "coverage": slice(10, 11), "weight": slice(11, 12)}


def _lib(be):
    return checked_lib(be, "the G-buffer pass has no oracle twin: the reference renders no G-buffer", "G-buffer", "ftn_gbuffer_abi_version",
                       A.FTN_GBUFFER_ABI_VERSION)


def resolve(be, raw):
    """ftn_gbuffer_resolve: raw [H, W, 12] sums -> dict of resolved [H, W, k] arrays (CHANNELS)."""
    lib = _lib(be)
    raw = np.ascontiguousarray(raw, dtype=np.float32)
    out = np.empty(raw.shape[:-1] + (12,), np.float32)
    be.check(lib.ftn_gbuffer_resolve(raw.ctypes.data_as(C.c_void_p), C.c_size_t(raw.size // 12), out.ctypes.data_as(C.c_void_p)))
    return {k: out[..., s] for k, s in CHANNELS.items()}


def render_gbuffer(be, builder, cam, res, sampler, tiles=None, crop=(0.0, 0.0, 1.0, 1.0), scene=None, raw=None,
                   pipeline=A.FTN_PIPELINE_AUTO, device=-1, film=None):
    """Shaped like scenes.render: create_scene (unless `scene` is given) + Film (unless `film` is given: a PBRT file's film with its
    crop window) + ftn_render_gbuffer.  `raw` ([H, W, 12] float32) is added into when given, else a zero buffer is.  Returns
    (resolved dict, raw sums, stats)."""
    lib = _lib(be)
    scene = scene or builder.create_scene()
    film = film or Film(be, res, crop)
    if raw is None:
        raw = np.zeros((film.height, film.width, 12), np.float32)
    if raw.shape != (film.height, film.width, 12) or raw.dtype != np.float32 or not raw.flags.c_contiguous:
        raise ValueError("raw must be a C-contiguous float32 array of shape %r" % ((film.height, film.width, 12),))
    args, keep = call_args(cam, film, None, sampler, tiles, pipeline, device)
    st = A.ftn_stats()
    be.check(lib.ftn_render_gbuffer(scene.handle, *args, raw.ctypes.data_as(C.c_void_p), C.byref(st)))
    return resolve(be, raw), raw, st.as_dict()


def render_gbuffer_torch(scene, cam, film, sampler, out, tiles=None, pipeline=A.FTN_PIPELINE_AUTO):
    """ftn_render_gbuffer_device into `out` (float32 CUDA tensor [H, W, 12], added into) on the current stream of its device."""
    import torch
    be = scene.be
    lib = _lib(be)
    _check_tensor(out, (film.height, film.width, 12))
    args, keep = call_args(cam, film, None, sampler, tiles, pipeline, out.device.index)
    st = A.ftn_stats()
    stream = torch.cuda.current_stream(out.device).cuda_stream
    be.check(lib.ftn_render_gbuffer_device(scene.handle, *args, C.c_void_p(out.data_ptr()), C.c_void_p(stream), C.byref(st)))
    return st.as_dict()


def resolve_torch(be, raw, out):
    """ftn_gbuffer_resolve_device: raw [..., 12] sums -> out [..., 12] resolved floats, both float32 CUDA tensors, current stream."""
    import torch
    lib = _lib(be)
    _check_tensor(raw, raw.shape)
    _check_tensor(out, raw.shape)
    if raw.shape[-1] != 12:
        raise ValueError("the last dimension holds the 12 floats of a pixel")
    stream = torch.cuda.current_stream(raw.device).cuda_stream
    be.check(lib.ftn_gbuffer_resolve_device(C.c_void_p(raw.data_ptr()), C.c_size_t(raw.numel() // 12), C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
    return out
