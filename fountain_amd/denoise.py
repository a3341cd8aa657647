"""Edge-avoiding a-trous denoiser (include/fountain_hip_denoise.h) over a resolved beauty image and its resolved first-hit G-buffer
(fountain_amd/gbuffer.py), for images rendered with few samples per pixel.

  denoise(be, rgb, gb12, params=None, device=-1)          host arrays in, host array out; the filter runs on the GPU
  denoise_cpu(be, rgb, gb12, params=None)                 the host twin, bit-identical to the GPU (for tests and tools)
  denoise_torch(be, rgb, gb12, out, workspace=None, params=None)   float32 CUDA tensors on the current stream

The variance-guided filter (include/fountain_hip_denoise_guided.h) also reads var4 [H, W, 4], the variance of each pixel's mean
(fountain_amd/moments.py: r, g, b, Y; Y is not read):

  denoise_guided(be, rgb, gb12, var4, params=None, device=-1)
  denoise_guided_cpu(be, rgb, gb12, var4, params=None)
  denoise_guided_torch(be, rgb, gb12, var4, out, workspace=None, params=None)

rgb is [H, W, 3] (ftn_film_resolve), gb12 is [H, W, 12] (ftn_gbuffer_resolve: albedo, normal, position, depth, coverage, weight).
`params` is an A.ftn_denoise_params (A.ftn_denoise_guided_params for the guided calls, guided_params), a dict of its fields (the others
keep their defaults), or None for the defaults.  The reference has no denoiser, so the CPU oracle has no twin of these calls.
"""
import ctypes as C

import numpy as np

from . import _abi as A
from ._nontwin import bind, check_tensor, check_workspace, current_stream, host_image, params_of, ptr, tptr


def _lib(be):
    return bind(be, A.EXTENSIONS["denoise"])


def _guided_lib(be):
    return bind(be, A.EXTENSIONS["denoise_guided"])


# the two filters: the params struct, the prefix of the C names, the library check.  The calls below are written once for both; the guided
# filter's take var4 between gb12 and the sizes
_PLAIN = (A.ftn_denoise_params, "ftn_denoise", _lib)
_GUIDED = (A.ftn_denoise_guided_params, "ftn_denoise_guided", _guided_lib)


def _params(be, kind, params):
    return params_of(be, params, kind[0], kind[1] + "_params_default", kind[2])


def default_params(be, **fields):
    """ftn_denoise_params_default, then the given fields."""
    return _params(be, _PLAIN, fields)


def guided_params(be, **fields):
    """ftn_denoise_guided_params_default, then the given fields."""
    return _params(be, _GUIDED, fields)


def _host_call(be, kind, suffix, rgb, gb12, var4, params, tail):
    lib = kind[2](be)
    p = _params(be, kind, params)
    try:
        rgb = host_image(rgb, 3)
        gb12 = host_image(gb12, 12, rgb.shape[:2])
    except ValueError:
        raise ValueError("expected rgb [H, W, 3] and gb12 [H, W, 12], got %r and %r" % (np.shape(rgb), np.shape(gb12))) from None
    images = [rgb, gb12]
    if kind is _GUIDED:
        try:
            images.append(host_image(var4, 4, rgb.shape[:2]))
        except ValueError:
            raise ValueError("expected var4 [H, W, 4] with the H and W of rgb %r, got %r" % (rgb.shape, np.shape(var4))) from None
    h, w = rgb.shape[:2]
    out = np.empty_like(rgb)
    be.check(getattr(lib, kind[1] + suffix)(*map(ptr, images), w, h, C.byref(p), ptr(out), *tail))
    return out


def denoise(be, rgb, gb12, params=None, device=-1):
    """ftn_denoise: host arrays, filtered on GPU `device` (-1 = the current one); returns a new [H, W, 3] float32 array."""
    return _host_call(be, _PLAIN, "", rgb, gb12, None, params, (device,))


def denoise_cpu(be, rgb, gb12, params=None):
    """ftn_denoise_cpu: the host twin of the filter (same bits as the GPU); returns a new [H, W, 3] float32 array."""
    return _host_call(be, _PLAIN, "_cpu", rgb, gb12, None, params, ())


def denoise_guided(be, rgb, gb12, var4, params=None, device=-1):
    """ftn_denoise_guided: host arrays, filtered on GPU `device` (-1 = the current one); returns a new [H, W, 3] float32 array."""
    return _host_call(be, _GUIDED, "", rgb, gb12, var4, params, (device,))


def denoise_guided_cpu(be, rgb, gb12, var4, params=None):
    """ftn_denoise_guided_cpu: the host twin of the guided filter (same bits as the GPU); returns a new [H, W, 3] float32 array."""
    return _host_call(be, _GUIDED, "_cpu", rgb, gb12, var4, params, ())


def _workspace_bytes(be, kind, w, h):
    n = C.c_size_t()
    be.check(getattr(kind[2](be), kind[1] + "_workspace_size")(w, h, C.byref(n)))
    return n.value


def workspace_bytes(be, w, h):
    """ftn_denoise_workspace_size: device bytes ftn_denoise_device needs for a w x h image (64 per pixel)."""
    return _workspace_bytes(be, _PLAIN, w, h)


def guided_workspace_bytes(be, w, h):
    """ftn_denoise_guided_workspace_size: device bytes ftn_denoise_guided_device needs for a w x h image (64 per pixel)."""
    return _workspace_bytes(be, _GUIDED, w, h)


def _torch_call(be, kind, rgb, gb12, var4, out, workspace, params):
    import torch
    lib = kind[2](be)
    p = _params(be, kind, params)
    inputs = [("rgb", rgb, 3), ("gb12", gb12, 12)] + ([("var4", var4, 4)] if kind is _GUIDED else [])
    for _, t, k in inputs + [("out", out, 3)]:
        try:
            check_tensor(t, tuple(np.shape(t)[:2]) + (k,))
        except ValueError:
            raise ValueError("expected contiguous float32 CUDA tensors %s and out [H, W, 3]"
                             % ", ".join("%s [H, W, %d]" % (n, k) for n, _, k in inputs)) from None
    h, w = rgb.shape[:2]
    if any(tuple(t.shape[:2]) != (h, w) or t.device != rgb.device for _, t, _ in inputs[1:] + [("out", out, 3)]):
        raise ValueError("%s and out must have the same H and W and live on the same device" % ", ".join(n for n, _, _ in inputs))
    need = _workspace_bytes(be, kind, w, h)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=rgb.device)
    else:
        check_workspace(workspace, need, rgb.device)
    be.check(getattr(lib, kind[1] + "_device")(*[tptr(t) for _, t, _ in inputs], w, h, C.byref(p),
                                               tptr(out), tptr(workspace), C.c_void_p(current_stream(rgb))))
    return out


def denoise_torch(be, rgb, gb12, out, workspace=None, params=None):
    """ftn_denoise_device: rgb [H, W, 3] and gb12 [H, W, 12] -> out [H, W, 3], contiguous float32 CUDA tensors on one device, on its
    current stream.  `workspace` is a CUDA tensor of at least workspace_bytes(be, W, H) bytes, 16-byte aligned; one is allocated when
    None (the call itself allocates nothing, so with a workspace given it can be captured in a graph).  Returns out."""
    return _torch_call(be, _PLAIN, rgb, gb12, None, out, workspace, params)


def denoise_guided_torch(be, rgb, gb12, var4, out, workspace=None, params=None):
    """ftn_denoise_guided_device: rgb [H, W, 3], gb12 [H, W, 12] and var4 [H, W, 4] -> out [H, W, 3], contiguous float32 CUDA tensors on
    one device, on its current stream.  `workspace` as for denoise_torch, of at least guided_workspace_bytes(be, W, H) bytes.  Returns
    out."""
    return _torch_call(be, _GUIDED, rgb, gb12, var4, out, workspace, params)
