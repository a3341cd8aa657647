"""Previous positions and screen-space motion (include/fountain_hip_motion.h): where the surface point each camera sample of ftn_render
sees was in the previous frame's scene, over exactly the G-buffer's samples, tiles and film.  With it temporal accumulation
(fountain_amd/temporal.py, `motion=`) follows objects that move through their transforms and meshes that deform.

  render_motion(be, builder, cam, res, sampler, scene=, prev_scene=)   host buffers -> (mv8 [H, W, 8], raw [H, W, 8] sums, stats)
  render_motion_torch(scene, prev_scene, cam, film, sampler, out)      adds into a float32 CUDA tensor [H, W, 8] on the current stream
  motion_resolve(be, raw) / motion_resolve_torch(be, raw, out)         sums -> mv8: position / H, normal / W, H / W, W
  motion_vectors(be, mv8, gb12, camera, prev_camera, film, device=-1)  [H, W, 2]: r_prev - r_cur in raster pixels, on the GPU
  motion_vectors_cpu(...) / motion_vectors_torch(..., out)             the host twin (same bits) / CUDA tensors on the current stream

The two scenes must correspond: the same primitives in the scene description's order, each of the same kind, spheres with the same
radius, z range, phi_max and orientation.  The raw layout is ftn_motion_pixel: prev_position 3, prev_normal 3, hit_weight, weight.  The
reference renders single frames, so the CPU oracle has no twin of these calls.
"""
import ctypes as C

import numpy as np

from . import _abi as A, _firsthit as F
from ._nontwin import bind, check_tensor as _check_tensor, current_stream, desc_of as _desc, host_image, ptr, tptr

# mv8 channels: name -> slice of the 8 floats ftn_motion_resolve writes per pixel
CHANNELS = {"prev_position": slice(0, 3), "prev_normal": slice(3, 6), "coverage": slice(6, 7), "weight": slice(7, 8)}
PASS = F.FirstHitPass(A.EXTENSIONS["motion"], 8, 8,
                      ("ftn_render_motion", "ftn_render_motion_device", "ftn_motion_resolve", "ftn_motion_resolve_device"), CHANNELS)


def _lib(be):
    return bind(be, PASS.ext)


def descs_differ(a, b):
    """The correspondence check of ftn_render_motion on two scene descriptions (ftn_scene_desc), before any scene is created: None when
    they correspond, else a sentence that names the first offending primitive."""
    if a.n_prims != b.n_prims:
        return "%d primitives against %d; primitive %d has no counterpart" % (a.n_prims, b.n_prims, min(a.n_prims, b.n_prims))
    if a.n_prims == 0:
        return None
    pa, pb = (np.ctypeslib.as_array(C.cast(d.prims, C.POINTER(A.c_u32)), (d.n_prims, 4)) for d in (a, b))
    kinds = np.nonzero(pa[:, 0] != pb[:, 0])[0]
    first_kind = int(kinds[0]) if len(kinds) else a.n_prims
    sphere_words = []
    for d in (a, b):       # radius, z_min, z_max, (theta_min, theta_max,) phi_max, reverse_orientation: words 64, 65, 66, 69, 70 of 72
        w = np.ctypeslib.as_array(C.cast(d.spheres, C.POINTER(A.c_u32)), (d.n_spheres, 72)) if d.n_spheres else np.zeros((0, 72), np.uint32)
        sphere_words.append(w[:, [64, 65, 66, 69, 70]])
    for i in np.nonzero(pa[:first_kind, 0] == A.FTN_SHAPE_SPHERE)[0]:
        if (sphere_words[0][pa[i, 1]] != sphere_words[1][pb[i, 1]]).any():
            return "primitive %d, a sphere, changed its radius, z range, phi_max or orientation (a sphere moves through its transforms only)" % i
    if first_kind < a.n_prims:
        return "primitive %d is of another kind in the previous scene" % first_kind
    return None


def motion_resolve(be, raw):
    """ftn_motion_resolve: raw [..., 8] sums -> mv8 [..., 8]."""
    return F.resolve_host(PASS, be, raw)


def render_motion(be, builder, cam, res, sampler, tiles=None, crop=(0.0, 0.0, 1.0, 1.0), scene=None, prev_scene=None, raw=None,
                  pipeline=A.FTN_PIPELINE_AUTO, device=-1, film=None):
    """Shaped like gbuffer.render_gbuffer: create_scene (unless `scene` is given) + Film (unless `film` is given) + ftn_render_motion
    against `prev_scene` (required: the previous frame's scene).  `raw` ([H, W, 8] float32) is added into when given, else a zero buffer
    is.  Returns (mv8, raw sums, stats)."""
    _lib(be)
    if prev_scene is None:
        raise ValueError("render_motion needs prev_scene, the previous frame's scene")
    raw, st = F.render_host(PASS, be, builder, cam, res, sampler, tiles=tiles, crop=crop, scene=scene, raw=raw, pipeline=pipeline, device=device, film=film,
                            lead=(prev_scene.handle,))
    return motion_resolve(be, raw), raw, st


def render_motion_torch(scene, prev_scene, cam, film, sampler, out, tiles=None, pipeline=A.FTN_PIPELINE_AUTO):
    """ftn_render_motion_device into `out` (float32 CUDA tensor [H, W, 8], added into) on the current stream of its device."""
    return F.render_torch(PASS, scene, cam, film, sampler, out, tiles=tiles, pipeline=pipeline, lead=(prev_scene.handle,))


def motion_resolve_torch(be, raw, out):
    """ftn_motion_resolve_device: raw [..., 8] sums -> out [..., 8], both float32 CUDA tensors, current stream."""
    return F.resolve_torch(PASS, be, raw, out)


def _host_vectors(be, fn, mv8, gb12, camera, prev_camera, film, tail):
    cam, pcam = _desc(camera, A.ftn_camera_desc, "camera"), _desc(prev_camera, A.ftn_camera_desc, "the previous camera")
    fd = _desc(film, A.ftn_film_desc, "film")
    mv8 = host_image(mv8, 8)
    gb12 = host_image(gb12, 12, mv8.shape[:2])
    h, w = mv8.shape[:2]
    out = np.empty((h, w, 2), np.float32)
    be.check(fn(ptr(mv8), ptr(gb12), C.byref(cam), C.byref(pcam), C.byref(fd), w, h, ptr(out), *tail))
    return out


def motion_vectors(be, mv8, gb12, camera, prev_camera, film, device=-1):
    """ftn_motion_vectors: host arrays, computed on GPU `device` (-1 = the current one); returns [H, W, 2]."""
    return _host_vectors(be, _lib(be).ftn_motion_vectors, mv8, gb12, camera, prev_camera, film, (int(device),))


def motion_vectors_cpu(be, mv8, gb12, camera, prev_camera, film):
    """ftn_motion_vectors_cpu: the host twin (same bits as the GPU); returns [H, W, 2]."""
    return _host_vectors(be, _lib(be).ftn_motion_vectors_cpu, mv8, gb12, camera, prev_camera, film, ())


def motion_vectors_torch(be, mv8, gb12, camera, prev_camera, film, out):
    """ftn_motion_vectors_device: mv8 [H, W, 8], gb12 [H, W, 12] -> out [H, W, 2], float32 CUDA tensors on one device, current stream."""
    import torch
    lib = _lib(be)
    cam, pcam = _desc(camera, A.ftn_camera_desc, "camera"), _desc(prev_camera, A.ftn_camera_desc, "the previous camera")
    fd = _desc(film, A.ftn_film_desc, "film")
    if not isinstance(mv8, torch.Tensor) or mv8.dim() != 3:
        raise ValueError("expected a contiguous float32 CUDA tensor mv8 [H, W, 8]")
    h, w = mv8.shape[:2]
    for t, k in ((mv8, 8), (gb12, 12), (out, 2)):
        _check_tensor(t, (h, w, k))
        if t.device != mv8.device:
            raise ValueError("every tensor must live on the device of mv8")
    be.check(lib.ftn_motion_vectors_device(tptr(mv8), tptr(gb12), C.byref(cam), C.byref(pcam), C.byref(fd), w, h,
                                           tptr(out), C.c_void_p(current_stream(mv8))))
    return out
