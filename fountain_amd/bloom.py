"""The bloom stage (include/fountain_hip_bloom.h): an HDR glare operator in linear light, between a resolved image and the display stage
-- a prefilter, a pyramid of 2:1 down-samplings, the same pyramid up again with the levels blended, and a composite that only moves
energy.

  BloomParams(be=None, karis=None, **fields)                           .desc is an ftn_bloom_params
  bloom(be, rgb, params=None, device=-1) / bloom_cpu(be, rgb, params=None)   -> float32 [H, W, 3]
  workspace_size(be, w, h, levels=None)                                -> bytes of device workspace bloom_device needs
  bloom_device(be, rgb_ptr, w, h, out_rgb_ptr, workspace_ptr, stream=0, params=None)
      device pointers on a stream (a hipStream_t as an integer); allocates nothing, does not synchronise, launches kernels only

`params` is a BloomParams, an A.ftn_bloom_params, a dict of BloomParams' arguments, or None for the defaults.  rgb is [H, W, 3] float32
(ftn_film_resolve).  bloom_cpu is the host twin, bit-identical to the GPU.  The reference writes linear OpenEXR files only, so the CPU
oracle has no twin of these calls.

  python -m fountain_amd.bloom in.exr -o out.exr [--strength S] [--levels N] [--scatter S] [--threshold T] [--knee K] [--karis]
blooms an existing OpenEXR file.
"""
import argparse
import ctypes as C
import sys

import numpy as np

from . import _abi as A
from ._cli import beside, refuse
from ._nontwin import bind, host_image, params_of, ptr, set_fields
from .api import default_backend


def _lib(be):
    return bind(be, A.EXTENSIONS["bloom"])


class BloomParams:
    def __init__(self, be=None, karis=None, **fields):
        """ftn_bloom_params_default, then the Karis flag and any other field of ftn_bloom_params (levels, strength, scatter, threshold,
        knee, clamp_max)."""
        self.be = be or default_backend()
        self.desc = A.ftn_bloom_params()
        _lib(self.be).ftn_bloom_params_default(C.byref(self.desc))
        if karis is not None:
            self.desc.flags = (self.desc.flags | A.FTN_BLOOM_KARIS) if karis else (self.desc.flags & ~A.FTN_BLOOM_KARIS)
        set_fields(self.desc, fields)


def _params(be, params):
    return params_of(be, params, A.ftn_bloom_params, "ftn_bloom_params_default", _lib, BloomParams)


def bloom(be, rgb, params=None, device=-1):
    """ftn_bloom: the bloomed image of a host image, computed on GPU `device`."""
    p = _params(be, params)
    rgb = host_image(rgb, 3)
    out = np.empty_like(rgb)
    be.check(_lib(be).ftn_bloom(ptr(rgb), rgb.shape[1], rgb.shape[0], C.byref(p), ptr(out), device))
    return out


def bloom_cpu(be, rgb, params=None):
    """ftn_bloom_cpu: the host twin (the same bits)."""
    p = _params(be, params)
    rgb = host_image(rgb, 3)
    out = np.empty_like(rgb)
    be.check(_lib(be).ftn_bloom_cpu(ptr(rgb), rgb.shape[1], rgb.shape[0], C.byref(p), ptr(out)))
    return out


def workspace_size(be, w, h, levels=None):
    """ftn_bloom_workspace_size: bytes of device workspace for a w x h image (levels None = the default)."""
    n = C.c_size_t(0)
    be.check(_lib(be).ftn_bloom_workspace_size(w, h, BloomParams(be).desc.levels if levels is None else levels, C.byref(n)))
    return n.value


def bloom_device(be, rgb_ptr, w, h, out_rgb_ptr, workspace_ptr, stream=0, params=None):
    """ftn_bloom_device: device pointers (rgb, out_rgb: 3 w h floats; workspace: workspace_size bytes), all 16-byte aligned, on `stream`.
    workspace_ptr may be 0 or None where the size is 0."""
    p = _params(be, params)
    be.check(_lib(be).ftn_bloom_device(C.c_void_p(rgb_ptr), w, h, C.byref(p), C.c_void_p(out_rgb_ptr), C.c_void_p(workspace_ptr or None), C.c_void_p(stream)))


def add_arguments(ap):
    """The bloom options shared by fountain_amd.render's and fountain_amd.display's command lines: --bloom switches the stage on and may
    carry the strength (opts.bloom is True for the flag alone)."""
    ap.add_argument("--bloom", type=float, nargs="?", const=True, default=None, metavar="STRENGTH",
                    help="bloom the linear image before the display stage (default strength 0.04)")
    ap.add_argument("--bloom-levels", type=int, default=None, metavar="N", help="the pyramid's depth, 0..12 (default 6)")
    ap.add_argument("--bloom-scatter", type=float, default=None, metavar="S", help="how much of each level comes from the coarser ones (default 0.7)")
    ap.add_argument("--bloom-threshold", type=float, default=None, metavar="T", help="luminance below which nothing blooms (default 0: everything)")
    ap.add_argument("--bloom-knee", type=float, default=None, metavar="K", help="the soft knee as a share of the threshold (default 0.5)")
    ap.add_argument("--bloom-karis", action="store_true", help="weight the first down-sampling by 1 / (1 + luminance): no single-pixel fireflies")


def bloom_options_given(opts):
    """The names of the bloom sub-options present in parsed arguments."""
    return [name for name, on in (("--bloom-levels", opts.bloom_levels is not None), ("--bloom-scatter", opts.bloom_scatter is not None),
                                  ("--bloom-threshold", opts.bloom_threshold is not None), ("--bloom-knee", opts.bloom_knee is not None),
                                  ("--bloom-karis", opts.bloom_karis)) if on]


def refusal(opts):
    """What is wrong with the bloom options of fountain_amd.render's or fountain_amd.display's parsed arguments, or None."""
    if opts.bloom is None:
        return "%s belongs to --bloom" % ", ".join(bloom_options_given(opts)) if bloom_options_given(opts) else None
    if opts.bloom is not True and not 0.0 <= opts.bloom <= 1.0:
        return "--bloom takes a strength in [0, 1]"
    return value_refusal(opts, "--bloom-")


def value_refusal(opts, prefix):
    """What is wrong with the values of the sub-options (the ranges of include/fountain_hip_bloom.h), or None; `prefix` names them."""
    if opts.bloom_levels is not None and not 0 <= opts.bloom_levels <= A.FTN_BLOOM_MAX_LEVELS:
        return "%slevels takes 0..%d" % (prefix, A.FTN_BLOOM_MAX_LEVELS)
    for name, v in (("scatter", opts.bloom_scatter), ("knee", opts.bloom_knee)):
        if v is not None and not 0.0 <= v <= 1.0:
            return "%s%s takes a value in [0, 1]" % (prefix, name)
    if opts.bloom_threshold is not None and not 0.0 <= opts.bloom_threshold < float("inf"):
        return "%sthreshold takes a finite value >= 0" % prefix
    return None


def params_from_arguments(be, opts, strength=None):
    """`strength`: this module's --strength; otherwise --bloom's value (the flag alone: the default strength)."""
    fields = {}
    given = getattr(opts, "bloom", None)
    if strength is None and given is not None and given is not True:
        strength = given
    for k, v in (("strength", strength), ("levels", opts.bloom_levels), ("scatter", opts.bloom_scatter), ("threshold", opts.bloom_threshold),
                 ("knee", opts.bloom_knee)):
        if v is not None:
            fields[k] = v
    return BloomParams(be, karis=True if opts.bloom_karis else None, **fields)


def main(argv=None):
    from .api import read_exr, write_exr
    ap = argparse.ArgumentParser(prog="fountain_amd.bloom")
    ap.add_argument("image", help="a linear-light OpenEXR file")
    ap.add_argument("-o", "--output", default=None, help="the bloomed OpenEXR file (default: the input's name with _bloom.exr)")
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--strength", type=float, default=None, metavar="S", help="how much of the image is replaced by its bloom (default 0.04)")
    for short, dest in (("--levels", "bloom_levels"), ("--scatter", "bloom_scatter"), ("--threshold", "bloom_threshold"), ("--knee", "bloom_knee")):
        ap.add_argument(short, dest=dest, type=int if short == "--levels" else float, default=None)
    ap.add_argument("--karis", dest="bloom_karis", action="store_true")
    opts = ap.parse_args(argv)
    out = opts.output or beside(opts.image, "_bloom.exr")
    if not out.endswith(".exr"):
        return refuse("the output must be an .exr file")
    if opts.strength is not None and not 0.0 <= opts.strength <= 1.0:
        return refuse("--strength must be in [0, 1]")
    if value_refusal(opts, "--"):
        return refuse(value_refusal(opts, "--"))
    be = default_backend()
    p = params_from_arguments(be, opts, opts.strength)
    write_exr(out, bloom(be, read_exr(opts.image, be), p, device=opts.gpu), be)
    print("bloom: %s (strength %.6g, %d levels)" % (out, p.desc.strength, p.desc.levels), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
