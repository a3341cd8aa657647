"""The display stage (include/fountain_hip_display.h): from a resolved linear-light image to pixels on a screen -- a luminance
histogram, a manual or automatic exposure, a tone curve, a transfer function, 8-bit codes with an optional ordered dither, and PNG.

  DisplayParams(be=None, tonemap="aces", transfer="srgb", dither=False, auto_exposure=False, **fields)   .desc is an ftn_display_params
  histogram(be, rgb, device=-1) / histogram_cpu(be, rgb)               -> uint32 [388]
  exposure(be, hist, params=None)                                      -> dict (scale, avg_log2, flags, the four counts); host only
  encode(be, rgb, scale, params=None, want_float=False, device=-1) / encode_cpu(...)   -> rgba8 uint32 [H, W] (, float32 [H, W, 3])
  display(be, rgb, params=None, want_float=False, device=-1) / display_cpu(...)        -> rgba8 (, float image), info: the whole chain
  histogram_device(be, rgb_ptr, w, h, hist_ptr, stream) / encode_device(be, rgb_ptr, w, h, scale, out_rgb_ptr, out_rgba8_ptr, stream,
      params=None)      device pointers on a stream (a hipStream_t as an integer); they allocate nothing and do not synchronise
  write_png(path, rgba8, be=None, gamma=None)                          8-bit RGB PNG; an sRGB chunk, or a gAMA chunk for a display gamma

`params` is a DisplayParams, an A.ftn_display_params, a dict of DisplayParams' arguments, or None for the defaults.  rgb is [H, W, 3]
float32 (ftn_film_resolve).  The *_cpu calls are the host twins, bit-identical to the GPU.  The reference writes linear OpenEXR files
only, so the CPU oracle has no twin of these calls.

  python -m fountain_amd.display in.exr -o out.png [--exposure EV | --auto-exposure] [--tonemap T] [--transfer T] [--gamma G] [--dither]
converts an existing OpenEXR file.  --bloom [STRENGTH] (with --bloom-levels, --bloom-scatter, --bloom-threshold, --bloom-knee and
--bloom-karis) blooms the linear image first (fountain_amd/bloom.py); the histogram, and so the automatic exposure, is the bloomed image's.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

from . import _abi as A
from ._cli import beside, refuse
from ._nontwin import bind, host_image, params_of, ptr, set_fields
from .api import default_backend

TONEMAPS = {"linear": A.FTN_DISPLAY_TONEMAP_LINEAR, "reinhard": A.FTN_DISPLAY_TONEMAP_REINHARD, "aces": A.FTN_DISPLAY_TONEMAP_ACES,
            "hable": A.FTN_DISPLAY_TONEMAP_HABLE}
TRANSFERS = {"srgb": A.FTN_DISPLAY_TRANSFER_SRGB, "gamma": A.FTN_DISPLAY_TRANSFER_GAMMA, "linear": A.FTN_DISPLAY_TRANSFER_LINEAR}


def _lib(be):
    return bind(be, A.EXTENSIONS["display"])


class DisplayParams:
    def __init__(self, be=None, tonemap=None, transfer=None, dither=None, auto_exposure=None, **fields):
        """ftn_display_params_default, then the curve and transfer by name, the two flags, and any other field of ftn_display_params
        (ev, key, white, gamma, p_lo, p_hi, min_ev, max_ev)."""
        self.be = be or default_backend()
        self.desc = A.ftn_display_params()
        _lib(self.be).ftn_display_params_default(C.byref(self.desc))
        if tonemap is not None:
            if tonemap not in TONEMAPS:
                raise ValueError("unknown tone curve %r: one of %s" % (tonemap, ", ".join(TONEMAPS)))
            self.desc.tonemap = TONEMAPS[tonemap]
        if transfer is not None:
            if transfer not in TRANSFERS:
                raise ValueError("unknown transfer %r: one of %s" % (transfer, ", ".join(TRANSFERS)))
            self.desc.transfer = TRANSFERS[transfer]
        for bit, on in ((A.FTN_DISPLAY_DITHER, dither), (A.FTN_DISPLAY_AUTO_EXPOSURE, auto_exposure)):
            if on is not None:
                self.desc.flags = (self.desc.flags | bit) if on else (self.desc.flags & ~bit)
        set_fields(self.desc, fields)

    @property
    def png_gamma(self):
        """What write_png's `gamma` should be for codes made with these parameters: None for sRGB, else the display gamma."""
        return {A.FTN_DISPLAY_TRANSFER_SRGB: None, A.FTN_DISPLAY_TRANSFER_GAMMA: float(self.desc.gamma), A.FTN_DISPLAY_TRANSFER_LINEAR: 1.0}[self.desc.transfer]


def _params(be, params):
    return params_of(be, params, A.ftn_display_params, "ftn_display_params_default", _lib, DisplayParams)


def histogram(be, rgb, device=-1):
    """ftn_display_histogram: the luminance histogram of a host image, counted on GPU `device`; uint32 [FTN_DISPLAY_HIST_WORDS]."""
    rgb = host_image(rgb, 3)
    hist = np.empty(A.FTN_DISPLAY_HIST_WORDS, np.uint32)
    be.check(_lib(be).ftn_display_histogram(ptr(rgb), rgb.shape[1], rgb.shape[0], ptr(hist), device))
    return hist


def histogram_cpu(be, rgb):
    """ftn_display_histogram_cpu: the host twin (the same words)."""
    rgb = host_image(rgb, 3)
    hist = np.empty(A.FTN_DISPLAY_HIST_WORDS, np.uint32)
    be.check(_lib(be).ftn_display_histogram_cpu(ptr(rgb), rgb.shape[1], rgb.shape[0], ptr(hist)))
    return hist


def histogram_device(be, rgb_ptr, w, h, hist_ptr, stream=0):
    """ftn_display_histogram_device: device pointers (rgb: 3 w h floats; hist: FTN_DISPLAY_HIST_WORDS words, cleared by the call), both
    16-byte aligned, on `stream`."""
    be.check(_lib(be).ftn_display_histogram_device(C.c_void_p(rgb_ptr), w, h, C.c_void_p(hist_ptr), C.c_void_p(stream)))


def exposure(be, hist, params=None):
    """ftn_display_exposure: the scale of `params` (2^ev, or in automatic mode from the histogram) and what it was made from, as a
    dict.  `hist` may be None in manual mode."""
    p = _params(be, params)
    if hist is not None:
        hist = np.ascontiguousarray(hist, dtype=np.uint32)
        if hist.shape != (A.FTN_DISPLAY_HIST_WORDS,):
            raise ValueError("expected a histogram of %d words" % A.FTN_DISPLAY_HIST_WORDS)
    info = A.ftn_display_info()
    be.check(_lib(be).ftn_display_exposure(ptr(hist), C.byref(p), C.byref(info)))
    return info.as_dict()


def _encode(be, fn, rgb, scale, params, want_float, tail):
    p = _params(be, params)
    rgb = host_image(rgb, 3)
    h, w = rgb.shape[:2]
    out8 = np.empty((h, w), np.uint32)
    outf = np.empty_like(rgb) if want_float else None
    be.check(fn(ptr(rgb), w, h, C.byref(p), scale, ptr(outf), ptr(out8), *tail))
    return (out8, outf) if want_float else out8


def encode(be, rgb, scale, params=None, want_float=False, device=-1):
    """ftn_display_encode: the 8-bit codes (uint32 [H, W]: R | G << 8 | B << 16 | 255 << 24) of a host image at the given scale,
    encoded on GPU `device`; with want_float also the display-referred float image."""
    return _encode(be, _lib(be).ftn_display_encode, rgb, scale, params, want_float, (device,))


def encode_cpu(be, rgb, scale, params=None, want_float=False):
    """ftn_display_encode_cpu: the host twin (the same bits)."""
    return _encode(be, _lib(be).ftn_display_encode_cpu, rgb, scale, params, want_float, ())


def encode_device(be, rgb_ptr, w, h, scale, out_rgb_ptr, out_rgba8_ptr, stream=0, params=None):
    """ftn_display_encode_device: device pointers (rgb and the optional out_rgb: 3 w h floats; out_rgba8: w h words), all 16-byte
    aligned, on `stream`.  out_rgb_ptr may be 0 or None."""
    p = _params(be, params)
    be.check(_lib(be).ftn_display_encode_device(C.c_void_p(rgb_ptr), w, h, C.byref(p), scale, C.c_void_p(out_rgb_ptr or None), C.c_void_p(out_rgba8_ptr),
                                                C.c_void_p(stream)))


def display(be, rgb, params=None, want_float=False, device=-1):
    """ftn_display: histogram (automatic mode only), exposure and encode of a host image on GPU `device`.  Returns (rgba8, info) or
    (rgba8, float image, info)."""
    lib = _lib(be)
    p = _params(be, params)
    rgb = host_image(rgb, 3)
    h, w = rgb.shape[:2]
    out8 = np.empty((h, w), np.uint32)
    outf = np.empty_like(rgb) if want_float else None
    info = A.ftn_display_info()
    be.check(lib.ftn_display(ptr(rgb), w, h, C.byref(p), ptr(outf), ptr(out8), C.byref(info), device))
    return (out8, outf, info.as_dict()) if want_float else (out8, info.as_dict())


def display_cpu(be, rgb, params=None, want_float=False):
    """The same chain on the host twins."""
    p = _params(be, params)
    info = exposure(be, histogram_cpu(be, rgb) if p.flags & A.FTN_DISPLAY_AUTO_EXPOSURE else None, p)
    out = encode_cpu(be, rgb, info["scale"], p, want_float)
    return (out[0], out[1], info) if want_float else (out, info)


def write_png(path, rgba8, be=None, gamma=None):
    """ftn_png_write: rgba8 (uint32 [H, W]) as an 8-bit RGB PNG file.  gamma None writes an sRGB chunk; a display gamma g (2.2, or 1 for
    linear codes) writes a gAMA chunk of 1 / g."""
    be = be or default_backend()
    rgba8 = np.ascontiguousarray(rgba8, dtype=np.uint32)
    if rgba8.ndim != 2:
        raise ValueError("expected rgba8 [H, W], got %r" % (rgba8.shape,))
    flags = 0 if gamma is None else ((int(100000.0 / gamma + 0.5) << 8) | A.FTN_PNG_GAMA)
    be.check(_lib(be).ftn_png_write(os.fsencode(path), ptr(rgba8), rgba8.shape[1], rgba8.shape[0], flags))


def add_arguments(ap):
    """The display options shared by this module's command line and fountain_amd.render's."""
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--exposure", type=float, default=None, metavar="EV", help="scale the image by 2^EV before the tone curve (default 0)")
    g.add_argument("--auto-exposure", action="store_true", help="take the exposure from the image's luminance histogram")
    ap.add_argument("--tonemap", default=None, choices=list(TONEMAPS), help="the tone curve (default aces)")
    ap.add_argument("--transfer", default=None, choices=list(TRANSFERS), help="the transfer function (default srgb)")
    ap.add_argument("--gamma", type=float, default=None, metavar="G", help="the display gamma of --transfer gamma (default 2.2)")
    ap.add_argument("--dither", action="store_true", help="ordered 8 x 8 dither of the 8-bit codes")


def display_options_given(opts):
    """The names of the display options (other than --png itself) present in parsed arguments."""
    return [name for name, on in (("--exposure", opts.exposure is not None), ("--auto-exposure", opts.auto_exposure), ("--tonemap", opts.tonemap is not None),
                                  ("--transfer", opts.transfer is not None), ("--gamma", opts.gamma is not None), ("--dither", opts.dither)) if on]


def params_from_arguments(be, opts):
    fields = {}
    if opts.exposure is not None:
        fields["ev"] = opts.exposure
    if opts.gamma is not None:
        fields["gamma"] = opts.gamma
    return DisplayParams(be, tonemap=opts.tonemap, transfer=opts.transfer, dither=opts.dither, auto_exposure=opts.auto_exposure, **fields)


def main(argv=None):
    from .api import read_exr
    ap = argparse.ArgumentParser(prog="fountain_amd.display")
    ap.add_argument("image", help="a linear-light OpenEXR file")
    ap.add_argument("-o", "--output", default=None, help="the PNG file (default: the input's name with .png)")
    ap.add_argument("--gpu", type=int, default=0)
    add_arguments(ap)
    from . import bloom as B
    B.add_arguments(ap)
    opts = ap.parse_args(argv)
    if B.refusal(opts):
        return refuse(B.refusal(opts))
    out = opts.output or beside(opts.image, ".png")
    if not out.endswith(".png"):
        return refuse("the output must be a .png file")
    if opts.gamma is not None and opts.transfer != "gamma":
        return refuse("--gamma belongs to --transfer gamma")
    be = default_backend()
    p = params_from_arguments(be, opts)
    img = read_exr(opts.image, be)
    if opts.bloom is not None:
        img = B.bloom(be, img, B.params_from_arguments(be, opts), device=opts.gpu)
    rgba8, info = display(be, img, p, device=opts.gpu)
    write_png(out, rgba8, be, p.png_gamma)
    print("display: %s (scale %.6g)" % (out, info["scale"]), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
