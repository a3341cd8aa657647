"""Helpers shared by the bindings of the calls the CPU oracle has no twin of (gbuffer.py, denoise.py, moments.py, adaptive.py)."""
import ctypes as C

from . import _abi as A
from .api import FountainError


def checked_lib(be, no_twin, what, abi_version_fn, abi_version):
    """be.lib, once it is the HIP library and reports the ABI version of `what` this binding was written for."""
    if be.is_oracle:
        raise FountainError(A.FTN_ERR_UNSUPPORTED, no_twin)
    have = getattr(be.lib, abi_version_fn)()
    if have != abi_version:
        raise FountainError(A.FTN_ERR_INTERNAL, "%s reports %s ABI version %d, this binding was written for %d: rebuild the library"
                            % (be.path, what, have, abi_version))
    return be.lib


def call_args(cam, film, integrator, sampler, tiles, pipeline, device, count_traffic=False):
    """The camera ... options arguments of a render call (no integrator argument when `integrator` is None), and what must stay alive."""
    tr = A.ftn_tile_range()
    tr.first, tr.stride, tr.count = tiles if tiles is not None else (0, 1, 0)
    opt = A.ftn_render_options()
    opt.pipeline, opt.device, opt.count_traffic = pipeline, device, int(count_traffic)
    args = [C.byref(cam.desc), C.byref(film.desc), C.byref(sampler.desc)] + ([C.byref(integrator.desc)] if integrator is not None else [])
    return args + [C.byref(tr), C.byref(opt)], (tr, opt)


def check_tensor(t, shape):
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError("expected a contiguous float32 CUDA tensor of shape %r" % (tuple(shape),))
