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
from ._nontwin import checked_lib


def _lib(be):
    return checked_lib(be, "the denoiser has no oracle twin: the reference has no denoiser", "denoise", "ftn_denoise_abi_version", A.FTN_DENOISE_ABI_VERSION)


def _guided_lib(be):
    return checked_lib(be, "the denoiser has no oracle twin: the reference has no denoiser", "guided denoise", "ftn_denoise_guided_abi_version",
                       A.FTN_DENOISE_GUIDED_ABI_VERSION)


def default_params(be, **fields):
    """ftn_denoise_params_default, then the given fields."""
    p = A.ftn_denoise_params()
    _lib(be).ftn_denoise_params_default(C.byref(p))
    for k, v in fields.items():
        if k not in dict(A.ftn_denoise_params._fields_):
            raise TypeError("ftn_denoise_params has no field %r" % k)
        setattr(p, k, v)
    return p


def _params(be, params):
    if params is None:
        return default_params(be)
    if isinstance(params, dict):
        return default_params(be, **params)
    if not isinstance(params, A.ftn_denoise_params):
        raise TypeError("params must be None, a dict or an ftn_denoise_params")
    return params


def _host_args(rgb, gb12):
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    gb12 = np.ascontiguousarray(gb12, dtype=np.float32)
    if rgb.ndim != 3 or rgb.shape[-1] != 3 or gb12.shape != rgb.shape[:2] + (12,):
        raise ValueError("expected rgb [H, W, 3] and gb12 [H, W, 12], got %r and %r" % (rgb.shape, gb12.shape))
    return rgb, gb12


def denoise(be, rgb, gb12, params=None, device=-1):
    """ftn_denoise: host arrays, filtered on GPU `device` (-1 = the current one); returns a new [H, W, 3] float32 array."""
    lib = _lib(be)
    p = _params(be, params)
    rgb, gb12 = _host_args(rgb, gb12)
    h, w = rgb.shape[:2]
    out = np.empty_like(rgb)
    be.check(lib.ftn_denoise(rgb.ctypes.data_as(C.c_void_p), gb12.ctypes.data_as(C.c_void_p), C.c_int32(w), C.c_int32(h), C.byref(p),
                             out.ctypes.data_as(C.c_void_p), C.c_int32(device)))
    return out


def denoise_cpu(be, rgb, gb12, params=None):
    """ftn_denoise_cpu: the host twin of the filter (same bits as the GPU); returns a new [H, W, 3] float32 array."""
    lib = _lib(be)
    p = _params(be, params)
    rgb, gb12 = _host_args(rgb, gb12)
    h, w = rgb.shape[:2]
    out = np.empty_like(rgb)
    be.check(lib.ftn_denoise_cpu(rgb.ctypes.data_as(C.c_void_p), gb12.ctypes.data_as(C.c_void_p), C.c_int32(w), C.c_int32(h), C.byref(p),
                                 out.ctypes.data_as(C.c_void_p)))
    return out


def workspace_bytes(be, w, h):
    """ftn_denoise_workspace_size: device bytes ftn_denoise_device needs for a w x h image (64 per pixel)."""
    n = C.c_size_t()
    be.check(_lib(be).ftn_denoise_workspace_size(C.c_int32(w), C.c_int32(h), C.byref(n)))
    return n.value


def denoise_torch(be, rgb, gb12, out, workspace=None, params=None):
    """ftn_denoise_device: rgb [H, W, 3] and gb12 [H, W, 12] -> out [H, W, 3], contiguous float32 CUDA tensors on one device, on its
    current stream.  `workspace` is a CUDA tensor of at least workspace_bytes(be, W, H) bytes, 16-byte aligned; one is allocated when
    None (the call itself allocates nothing, so with a workspace given it can be captured in a graph).  Returns out."""
    import torch
    lib = _lib(be)
    p = _params(be, params)
    for t, k in ((rgb, 3), (gb12, 12), (out, 3)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.dim() != 3 or t.shape[-1] != k:
            raise ValueError("expected contiguous float32 CUDA tensors rgb [H, W, 3], gb12 [H, W, 12] and out [H, W, 3]")
    h, w = rgb.shape[:2]
    if tuple(gb12.shape[:2]) != (h, w) or tuple(out.shape[:2]) != (h, w) or gb12.device != rgb.device or out.device != rgb.device:
        raise ValueError("rgb, gb12 and out must have the same H and W and live on the same device")
    need = workspace_bytes(be, w, h)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=rgb.device)
    elif not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or not workspace.is_contiguous() or workspace.device != rgb.device \
            or workspace.numel() * workspace.element_size() < need:
        raise ValueError("workspace must be a contiguous CUDA tensor of at least %d bytes on the device of rgb" % need)
    stream = torch.cuda.current_stream(rgb.device).cuda_stream
    be.check(lib.ftn_denoise_device(C.c_void_p(rgb.data_ptr()), C.c_void_p(gb12.data_ptr()), C.c_int32(w), C.c_int32(h), C.byref(p),
                                    C.c_void_p(out.data_ptr()), C.c_void_p(workspace.data_ptr()), C.c_void_p(stream)))
    return out


# ------------------------------------------------------------------ the variance-guided filter
def guided_params(be, **fields):
    """ftn_denoise_guided_params_default, then the given fields."""
    p = A.ftn_denoise_guided_params()
    _guided_lib(be).ftn_denoise_guided_params_default(C.byref(p))
    for k, v in fields.items():
        if k not in dict(A.ftn_denoise_guided_params._fields_):
            raise TypeError("ftn_denoise_guided_params has no field %r" % k)
        setattr(p, k, v)
    return p


def _guided_params(be, params):
    if params is None:
        return guided_params(be)
    if isinstance(params, dict):
        return guided_params(be, **params)
    if not isinstance(params, A.ftn_denoise_guided_params):
        raise TypeError("params must be None, a dict or an ftn_denoise_guided_params")
    return params


def _guided_host_args(rgb, gb12, var4):
    rgb, gb12 = _host_args(rgb, gb12)
    var4 = np.ascontiguousarray(var4, dtype=np.float32)
    if var4.shape != rgb.shape[:2] + (4,):
        raise ValueError("expected var4 [H, W, 4] with the H and W of rgb %r, got %r" % (rgb.shape, var4.shape))
    return rgb, gb12, var4


def denoise_guided(be, rgb, gb12, var4, params=None, device=-1):
    """ftn_denoise_guided: host arrays, filtered on GPU `device` (-1 = the current one); returns a new [H, W, 3] float32 array."""
    lib = _guided_lib(be)
    p = _guided_params(be, params)
    rgb, gb12, var4 = _guided_host_args(rgb, gb12, var4)
    h, w = rgb.shape[:2]
    out = np.empty_like(rgb)
    be.check(lib.ftn_denoise_guided(rgb.ctypes.data_as(C.c_void_p), gb12.ctypes.data_as(C.c_void_p), var4.ctypes.data_as(C.c_void_p),
                                    C.c_int32(w), C.c_int32(h), C.byref(p), out.ctypes.data_as(C.c_void_p), C.c_int32(device)))
    return out


def denoise_guided_cpu(be, rgb, gb12, var4, params=None):
    """ftn_denoise_guided_cpu: the host twin of the guided filter (same bits as the GPU); returns a new [H, W, 3] float32 array."""
    lib = _guided_lib(be)
    p = _guided_params(be, params)
    rgb, gb12, var4 = _guided_host_args(rgb, gb12, var4)
    h, w = rgb.shape[:2]
    out = np.empty_like(rgb)
    be.check(lib.ftn_denoise_guided_cpu(rgb.ctypes.data_as(C.c_void_p), gb12.ctypes.data_as(C.c_void_p), var4.ctypes.data_as(C.c_void_p),
                                        C.c_int32(w), C.c_int32(h), C.byref(p), out.ctypes.data_as(C.c_void_p)))
    return out


def guided_workspace_bytes(be, w, h):
    """ftn_denoise_guided_workspace_size: device bytes ftn_denoise_guided_device needs for a w x h image (64 per pixel)."""
    n = C.c_size_t()
    be.check(_guided_lib(be).ftn_denoise_guided_workspace_size(C.c_int32(w), C.c_int32(h), C.byref(n)))
    return n.value


def denoise_guided_torch(be, rgb, gb12, var4, out, workspace=None, params=None):
    """ftn_denoise_guided_device: rgb [H, W, 3], gb12 [H, W, 12] and var4 [H, W, 4] -> out [H, W, 3], contiguous float32 CUDA tensors on
    one device, on its current stream.  `workspace` as for denoise_torch, of at least guided_workspace_bytes(be, W, H) bytes.  Returns
    out."""
    import torch
    lib = _guided_lib(be)
    p = _guided_params(be, params)
    for t, k in ((rgb, 3), (gb12, 12), (var4, 4), (out, 3)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.dim() != 3 or t.shape[-1] != k:
            raise ValueError("expected contiguous float32 CUDA tensors rgb [H, W, 3], gb12 [H, W, 12], var4 [H, W, 4] and out [H, W, 3]")
    h, w = rgb.shape[:2]
    if any(tuple(t.shape[:2]) != (h, w) or t.device != rgb.device for t in (gb12, var4, out)):
        raise ValueError("rgb, gb12, var4 and out must have the same H and W and live on the same device")
    need = guided_workspace_bytes(be, w, h)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=rgb.device)
    elif not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or not workspace.is_contiguous() or workspace.device != rgb.device \
            or workspace.numel() * workspace.element_size() < need:
        raise ValueError("workspace must be a contiguous CUDA tensor of at least %d bytes on the device of rgb" % need)
    stream = torch.cuda.current_stream(rgb.device).cuda_stream
    be.check(lib.ftn_denoise_guided_device(C.c_void_p(rgb.data_ptr()), C.c_void_p(gb12.data_ptr()), C.c_void_p(var4.data_ptr()), C.c_int32(w),
                                           C.c_int32(h), C.byref(p), C.c_void_p(out.data_ptr()), C.c_void_p(workspace.data_ptr()), C.c_void_p(stream)))
    return out
