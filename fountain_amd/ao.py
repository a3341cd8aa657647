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

from . import _abi as A, _firsthit as F
from ._nontwin import bind, ptr

# resolved channels: name -> slice of the 6 floats ftn_ao_resolve writes per pixel
CHANNELS = {"ao": slice(0, 1), "bent": slice(1, 4), "coverage": slice(4, 5), "weight": slice(5, 6)}
PASS = F.FirstHitPass(A.EXTENSIONS["ao"], 8, 6, ("ftn_render_ao", "ftn_render_ao_device", "ftn_ao_resolve", "ftn_ao_resolve_device"), CHANNELS)
INF = float("inf")


def _lib(be):
    return bind(be, PASS.ext)


def options(rays=4, radius=INF):
    o = A.ftn_ao_options()
    o.rays, o.radius = int(rays), float(radius)
    return o


def resolve(be, raw, rays):
    """ftn_ao_resolve: raw [H, W, 8] sums -> dict of resolved [H, W, k] arrays (CHANNELS)."""
    return F.channels(PASS, F.resolve_host(PASS, be, raw, lambda: (int(rays),)))


def ao_rays(be, hit24, u2, radius=INF):
    """ftn_ao_rays: for n interaction records in ftn_intersect_full's layout ([n, 24]) and n pairs of draws ([n, 2]), the occlusion rays
    [n, 8] = {o, d, t_max = radius, 0} the pass builds.  Runs on the host, no GPU needed."""
    lib = _lib(be)
    hit24 = np.ascontiguousarray(hit24, dtype=np.float32).reshape(-1, 24)
    u2 = np.ascontiguousarray(u2, dtype=np.float32).reshape(-1, 2)
    if len(hit24) != len(u2):
        raise ValueError("one pair of draws per interaction record")
    out = np.empty((len(hit24), 8), np.float32)
    be.check(lib.ftn_ao_rays(ptr(hit24), ptr(u2), len(hit24), float(radius), ptr(out)))
    return out


def render_ao(be, builder, cam, res, sampler, rays=4, radius=INF, tiles=None, crop=(0.0, 0.0, 1.0, 1.0), scene=None, raw=None,
              pipeline=A.FTN_PIPELINE_AUTO, device=-1, film=None, count_traffic=False):
    """Shaped like gbuffer.render_gbuffer: create_scene (unless `scene` is given) + Film (unless `film` is given) + ftn_render_ao.  `raw`
    ([H, W, 8] float32) is added into when given, else a zero buffer is.  count_traffic: the occlusion rays take the reference-order
    traversal instead of the production any-hit kernels.  Returns (resolved dict, raw sums, stats)."""
    raw, st = F.render_host(PASS, be, builder, cam, res, sampler, tiles=tiles, crop=crop, scene=scene, raw=raw, pipeline=pipeline, device=device, film=film,
                            count_traffic=count_traffic, extra=lambda: (C.byref(options(rays, radius)),))
    return resolve(be, raw, rays), raw, st


def render_ao_torch(scene, cam, film, sampler, out, rays=4, radius=INF, tiles=None, pipeline=A.FTN_PIPELINE_AUTO):
    """ftn_render_ao_device into `out` (float32 CUDA tensor [H, W, 8], added into) on the current stream of its device."""
    return F.render_torch(PASS, scene, cam, film, sampler, out, tiles=tiles, pipeline=pipeline, extra=lambda: (C.byref(options(rays, radius)),))


def resolve_torch(be, raw, rays, out):
    """ftn_ao_resolve_device: raw [..., 8] sums -> out [..., 6] resolved floats, both float32 CUDA tensors, current stream."""
    return F.resolve_torch(PASS, be, raw, out, lambda: (int(rays),))
