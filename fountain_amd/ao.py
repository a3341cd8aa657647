"""Ambient occlusion and bent normals (include/fountain_hip_ao.h) over exactly the camera samples ftn_render traces for the same sampler,
tiles and film: per recorded surface `rays` cosine-distributed occlusion rays of length `radius` through the production any-hit kernels.

  render_ao(be, builder, cam, res, sampler, rays=4, radius=inf)   host buffers -> (resolved dict of [H, W, k] arrays, raw [H, W, 8] sums, stats)
  render_ao_torch(scene, cam, film, sampler, out, rays, radius)   adds into a float32 CUDA tensor [H, W, 8] on the current stream
  resolve(be, raw, rays) / resolve_torch(be, raw, rays, out)      sums -> the 6 resolved floats per pixel
  ao_rays(be, hit24, u2, radius)                                  the occlusion rays of interaction records, on the host

The raw layout is ftn_ao_pixel: open, bent 3, hit_weight, weight, two words of padding.  The reference has no ambient-occlusion
integrator, so the CPU oracle has no twin of these calls.
"""
import ctypes as C

import numpy as np

from . import _abi as A
from ._nontwin import call_args, check_tensor as _check_tensor, checked_lib
from .api import Film

# resolved channels: name -> slice of the 6 floats ftn_ao_resolve writes per pixel
CHANNELS = {"ao": slice(0, 1), "bent": slice(1, 4), "coverage": slice(4, 5), "weight": slice(5, 6)}
INF = float("inf")


def _lib(be):
    lib = checked_lib(be, "the ambient-occlusion pass has no oracle twin: the reference has no such integrator", "ambient-occlusion",
                      "ftn_ao_abi_version", A.FTN_AO_ABI_VERSION)
    for name, (argtypes, restype) in A.AO_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, restype
    return lib


def options(rays=4, radius=INF):
    o = A.ftn_ao_options()
    o.rays, o.radius = int(rays), float(radius)
    return o


def resolve(be, raw, rays):
    """ftn_ao_resolve: raw [H, W, 8] sums -> dict of resolved [H, W, k] arrays (CHANNELS)."""
    lib = _lib(be)
    raw = np.ascontiguousarray(raw, dtype=np.float32)
    if raw.shape[-1] != 8:
        raise ValueError("the last dimension holds the 8 floats of a pixel")
    out = np.empty(raw.shape[:-1] + (6,), np.float32)
    be.check(lib.ftn_ao_resolve(raw.ctypes.data_as(C.c_void_p), raw.size // 8, int(rays), out.ctypes.data_as(C.c_void_p)))
    return {k: out[..., s] for k, s in CHANNELS.items()}


def ao_rays(be, hit24, u2, radius=INF):
    """ftn_ao_rays: for n interaction records in ftn_intersect_full's layout ([n, 24]) and n pairs of draws ([n, 2]), the occlusion rays
    [n, 8] = {o, d, t_max = radius, 0} the pass builds.  Runs on the host, no GPU needed."""
    lib = _lib(be)
    hit24 = np.ascontiguousarray(hit24, dtype=np.float32).reshape(-1, 24)
    u2 = np.ascontiguousarray(u2, dtype=np.float32).reshape(-1, 2)
    if len(hit24) != len(u2):
        raise ValueError("one pair of draws per interaction record")
    out = np.empty((len(hit24), 8), np.float32)
    be.check(lib.ftn_ao_rays(hit24.ctypes.data_as(C.c_void_p), u2.ctypes.data_as(C.c_void_p), len(hit24), float(radius), out.ctypes.data_as(C.c_void_p)))
    return out


def render_ao(be, builder, cam, res, sampler, rays=4, radius=INF, tiles=None, crop=(0.0, 0.0, 1.0, 1.0), scene=None, raw=None,
              pipeline=A.FTN_PIPELINE_AUTO, device=-1, film=None, count_traffic=False):
    """Shaped like gbuffer.render_gbuffer: create_scene (unless `scene` is given) + Film (unless `film` is given) + ftn_render_ao.  `raw`
    ([H, W, 8] float32) is added into when given, else a zero buffer is.  count_traffic: the occlusion rays take the reference-order
    traversal instead of the production any-hit kernels.  Returns (resolved dict, raw sums, stats)."""
    lib = _lib(be)
    scene = scene or builder.create_scene()
    film = film or Film(be, res, crop)
    if raw is None:
        raw = np.zeros((film.height, film.width, 8), np.float32)
    if raw.shape != (film.height, film.width, 8) or raw.dtype != np.float32 or not raw.flags.c_contiguous:
        raise ValueError("raw must be a C-contiguous float32 array of shape %r" % ((film.height, film.width, 8),))
    args, keep = call_args(cam, film, None, sampler, tiles, pipeline, device, count_traffic)
    st, opt = A.ftn_stats(), options(rays, radius)
    be.check(lib.ftn_render_ao(scene.handle, *args, C.byref(opt), raw.ctypes.data_as(C.c_void_p), C.byref(st)))
    return resolve(be, raw, rays), raw, st.as_dict()


def render_ao_torch(scene, cam, film, sampler, out, rays=4, radius=INF, tiles=None, pipeline=A.FTN_PIPELINE_AUTO):
    """ftn_render_ao_device into `out` (float32 CUDA tensor [H, W, 8], added into) on the current stream of its device."""
    import torch
    be = scene.be
    lib = _lib(be)
    _check_tensor(out, (film.height, film.width, 8))
    args, keep = call_args(cam, film, None, sampler, tiles, pipeline, out.device.index)
    st, opt = A.ftn_stats(), options(rays, radius)
    stream = torch.cuda.current_stream(out.device).cuda_stream
    be.check(lib.ftn_render_ao_device(scene.handle, *args, C.byref(opt), C.c_void_p(out.data_ptr()), C.c_void_p(stream), C.byref(st)))
    return st.as_dict()


def resolve_torch(be, raw, rays, out):
    """ftn_ao_resolve_device: raw [..., 8] sums -> out [..., 6] resolved floats, both float32 CUDA tensors, current stream."""
    import torch
    lib = _lib(be)
    _check_tensor(raw, raw.shape)
    if raw.shape[-1] != 8:
        raise ValueError("the last dimension holds the 8 floats of a pixel")
    _check_tensor(out, tuple(raw.shape[:-1]) + (6,))
    stream = torch.cuda.current_stream(raw.device).cuda_stream
    be.check(lib.ftn_ao_resolve_device(C.c_void_p(raw.data_ptr()), raw.numel() // 8, int(rays), C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
    return out
