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

from . import _abi as A, _firsthit as F
from ._nontwin import bind, check_tensor as _check_tensor, current_stream, ptr, tptr

# resolved channels: name -> slice of the 12 floats ftn_gbuffer_resolve writes per pixel
CHANNELS = {"albedo": slice(0, 3), "normal": slice(3, 6), "position": slice(6, 9), "depth": slice(9, 10),
            "coverage": slice(10, 11), "weight": slice(11, 12)}
PASS = F.FirstHitPass(A.EXTENSIONS["gbuffer"], 12, 12,
                      ("ftn_render_gbuffer", "ftn_render_gbuffer_device", "ftn_gbuffer_resolve", "ftn_gbuffer_resolve_device"), CHANNELS)


def _lib(be):
    return bind(be, PASS.ext)


def resolve(be, raw):
    """ftn_gbuffer_resolve: raw [H, W, 12] sums -> dict of resolved [H, W, k] arrays (CHANNELS).  (Written out: unlike the other passes'
    it takes any array of a multiple of 12 floats, whatever its last dimension.)"""
    lib = _lib(be)
    raw = np.ascontiguousarray(raw, dtype=np.float32)
    out = np.empty(raw.shape[:-1] + (12,), np.float32)
    be.check(lib.ftn_gbuffer_resolve(ptr(raw), raw.size // 12, ptr(out)))
    return F.channels(PASS, out)


def render_gbuffer(be, builder, cam, res, sampler, tiles=None, crop=(0.0, 0.0, 1.0, 1.0), scene=None, raw=None,
                   pipeline=A.FTN_PIPELINE_AUTO, device=-1, film=None):
    """Shaped like scenes.render: create_scene (unless `scene` is given) + Film (unless `film` is given: a PBRT file's film with its
    crop window) + ftn_render_gbuffer.  `raw` ([H, W, 12] float32) is added into when given, else a zero buffer is.  Returns
    (resolved dict, raw sums, stats)."""
    raw, st = F.render_host(PASS, be, builder, cam, res, sampler, tiles=tiles, crop=crop, scene=scene, raw=raw, pipeline=pipeline, device=device, film=film)
    return resolve(be, raw), raw, st


def render_gbuffer_torch(scene, cam, film, sampler, out, tiles=None, pipeline=A.FTN_PIPELINE_AUTO):
    """ftn_render_gbuffer_device into `out` (float32 CUDA tensor [H, W, 12], added into) on the current stream of its device."""
    return F.render_torch(PASS, scene, cam, film, sampler, out, tiles=tiles, pipeline=pipeline)


def resolve_torch(be, raw, out):
    """ftn_gbuffer_resolve_device: raw [..., 12] sums -> out [..., 12] resolved floats, both float32 CUDA tensors, current stream.
    (Written out: it checks `out` before the last dimension.)"""
    lib = _lib(be)
    _check_tensor(raw, raw.shape)
    _check_tensor(out, raw.shape)
    if raw.shape[-1] != 12:
        raise ValueError("the last dimension holds the 12 floats of a pixel")
    be.check(lib.ftn_gbuffer_resolve_device(tptr(raw), raw.numel() // 12, tptr(out), C.c_void_p(current_stream(raw))))
    return out
