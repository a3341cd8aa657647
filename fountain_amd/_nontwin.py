"""Helpers shared by the bindings of the calls the CPU oracle has no twin of: the render passes (gbuffer.py, ao.py, motion.py, lightpass.py
-- through _firsthit.py -- and idmatte.py, moments.py, adaptive.py, filters.py), the image-space stages (denoise.py, temporal.py, display.py,
bloom.py, vectorblur.py, metrics.py, motion.py's vectors, lightpass.py's compose) and subdiv.py.  bind() is the one place where the
functions of an extension header get their argument and result types."""
import ctypes as C

import numpy as np

from . import _abi as A
from .api import FountainError


def bind(be, ext):
    """be.lib, once it is the HIP library and reports the ABI version of the extension `ext` (an A.Extension) this binding was written
    for.  The first call for a library that passes asks for the version and gives the extension's functions their prototypes; be.bound
    remembers that (a loaded library does not change), so later calls only look the header up there."""
    if be.is_oracle:
        raise FountainError(A.FTN_ERR_UNSUPPORTED, ext.no_twin)
    if ext.header not in be.bound:
        have = getattr(be.lib, ext.abi_version_fn)()
        if have != ext.abi_version:
            raise FountainError(A.FTN_ERR_INTERNAL, "%s reports %s ABI version %d, this binding was written for %d: rebuild the library"
                                % (be.path, ext.what, have, ext.abi_version))
        for name, (argtypes, restype) in ext.prototypes.items():
            fn = getattr(be.lib, name)
            fn.argtypes, fn.restype = argtypes, restype
        be.bound.add(ext.header)
    return be.lib


def call_args(cam, film, integrator, sampler, tiles, pipeline, device, count_traffic=False):
    """The camera ... options arguments of a render call (no integrator argument when `integrator` is None), and what must stay alive."""
    tr = A.ftn_tile_range()
    tr.first, tr.stride, tr.count = tiles if tiles is not None else (0, 1, 0)
    opt = A.ftn_render_options()
    opt.pipeline, opt.device, opt.count_traffic = pipeline, device, int(count_traffic)
    args = [C.byref(cam.desc), C.byref(film.desc), C.byref(sampler.desc)] + ([C.byref(integrator.desc)] if integrator is not None else [])
    return args + [C.byref(tr), C.byref(opt)], (tr, opt)


def index_list(indices):
    """An optional list of indices as the (uint32 array pointer or None, length) pair of a C call (the pointer keeps its array alive):
    None stays None with length 0 (lightpass.py: all lights)."""
    if indices is None:
        return None, 0
    a = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
    return ptr(a), len(a)


def check_tensor(t, shape):
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError("expected a contiguous float32 CUDA tensor of shape %r" % (tuple(shape),))


def current_stream(t):
    """The current stream of tensor t's device, as the integer a C call takes."""
    import torch
    return torch.cuda.current_stream(t.device).cuda_stream


def check_array(a, shape, what):
    if a.shape != shape or a.dtype != np.float32 or not a.flags.c_contiguous:
        raise ValueError("%s must be a C-contiguous float32 array of shape %r" % (what, shape))


def desc_of(obj, typ, what):
    """`obj` as the descriptor struct `typ`: the struct itself, or what carries one as .desc (a camera, a film); TypeError otherwise."""
    d = obj if isinstance(obj, typ) else getattr(obj, "desc", None)
    if not isinstance(d, typ):
        raise TypeError("%s must be a %s or carry one as .desc" % (what, typ.__name__))
    return d


def check_workspace(t, need, device):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous() or t.device != device or t.numel() * t.element_size() < need:
        raise ValueError("workspace must be a contiguous CUDA tensor of at least %d bytes on the device of rgb" % need)


def set_fields(p, fields, hidden=()):
    """The given fields of the params struct p (`hidden`: fields a caller does not set); returns p."""
    for k, v in fields.items():
        if k not in dict(p._fields_) or k in hidden:
            raise TypeError("%s has no field %r" % (type(p).__name__, k))
        setattr(p, k, v)
    return p


def params_of(be, params, struct, default_fn_name, lib_fn, wrapper=None, hidden=()):
    """A `struct` from what a call takes as `params`: None (the defaults of lib_fn(be)'s default_fn_name), a dict (the defaults, then its
    fields -- the arguments of `wrapper`, where the stage has one: a class whose instances carry the struct as .desc), a wrapper, or a
    struct, which is returned as it is."""
    if params is None or isinstance(params, dict):
        if wrapper is not None:
            return wrapper(be, **(params or {})).desc
        p = struct()
        getattr(lib_fn(be), default_fn_name)(C.byref(p))
        return set_fields(p, params or {}, hidden)
    if wrapper is not None and isinstance(params, wrapper):
        return params.desc
    if not isinstance(params, struct):
        raise TypeError("params must be None, a dict%s or an %s" % (", a %s" % wrapper.__name__ if wrapper else "", struct.__name__))
    return params


_IMAGES = {3: "rgb", 4: "var4", 8: "history", 12: "gb12"}


def host_image(a, channels, hw=None):
    """`a` as a contiguous float32 [H, W, channels] array (with H, W = hw when given); ValueError otherwise."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 3 or a.shape[-1] != channels or (hw is not None and a.shape[:2] != tuple(hw)):
        raise ValueError("expected %s [H, W, %d], got %r" % (_IMAGES[channels], channels, a.shape))
    return a


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def tptr(t):
    """The device pointer of a tensor (None stays None)."""
    return None if t is None else C.c_void_p(t.data_ptr())
