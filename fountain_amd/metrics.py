"""The measuring stage (include/fountain_hip_metrics.h): two resolved images in, the standard rendering error measures out -- MSE, RMSE,
MAE, relMSE, SMAPE, PSNR, the largest difference and, on request, SSIM -- per image, per 16 x 16 film tile and per pixel.

  MetricsParams(be=None, ssim=None, **fields)                            .desc is an ftn_metrics_params
  compare(be, test, ref, params=None, device=-1, error_map=False, ssim_map=False, tile_sums=False, totals=False)
  compare_cpu(be, test, ref, params=None, error_map=False, ssim_map=False, tile_sums=False, totals=False)
      -> a dict of the fields of ftn_metrics_result (mse_rgb a tuple), and where asked "error_map" and "ssim_map" (float32 [H, W]),
         "tile_sums" (float64 [n_tiles, 8]: SE, AE, REL, SM, SE_r, SE_g, SE_b, SSIM) and "totals" (a dict of ftn_metrics_totals)
  workspace_size(be, w, h, flags=0)                                      -> bytes of device workspace compare_device needs
  compare_device(be, test_ptr, ref_ptr, w, h, totals_ptr, workspace_ptr, stream=0, params=None, error_map_ptr=0, ssim_map_ptr=0, tile_sums_ptr=0)
      device pointers on a stream (a hipStream_t as an integer); allocates nothing, does not synchronise, launches kernels only;
      resolve(be, totals, params) turns the downloaded ftn_metrics_totals into the dict
  ssim_weights(be)                                                       -> the 11 normalised weights of the SSIM window

`params` is a MetricsParams, an A.ftn_metrics_params, a dict of MetricsParams' arguments, or None for the defaults.  test and ref are
[H, W, 3] float32 (ftn_film_resolve).  compare_cpu is the host twin, bit-identical to the GPU.  The reference compares no images, so
the CPU oracle has no twin of these calls.

  python -m fountain_amd.metrics test.exr ref.exr [--ssim] [--peak P] [--rel-eps E] [--error-map F.exr] [--ssim-map F.exr] [--tile-map F.exr]
                                 [--json] [--cpu] [--gpu N] [--fail-above NAME=VALUE ...]
compares two OpenEXR files: exit code 0 when every threshold holds, 1 when a named metric exceeds its value or is NaN, 2 for usage
errors and sizes that differ (nothing is written then).
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

from . import _abi as A
from ._cli import refuse
from ._nontwin import bind, host_image, params_of, ptr, set_fields
from .api import default_backend

RESULT_FIELDS = tuple(name for name, _ in A.ftn_metrics_result._fields_)
SUMS = ("SE", "AE", "REL", "SM", "SE_r", "SE_g", "SE_b", "SSIM")


def _lib(be):
    return bind(be, A.EXTENSIONS["metrics"])


class MetricsParams:
    def __init__(self, be=None, ssim=None, **fields):
        """ftn_metrics_params_default, then the SSIM flag and any other field of ftn_metrics_params (peak, rel_eps)."""
        self.be = be or default_backend()
        self.desc = A.ftn_metrics_params()
        _lib(self.be).ftn_metrics_params_default(C.byref(self.desc))
        if ssim is not None:
            self.desc.flags = (self.desc.flags | A.FTN_METRICS_SSIM) if ssim else (self.desc.flags & ~A.FTN_METRICS_SSIM)
        set_fields(self.desc, fields)


def _params(be, params):
    return params_of(be, params, A.ftn_metrics_params, "ftn_metrics_params_default", _lib, MetricsParams)


def _struct_dict(s):
    return {name: (tuple(v) if hasattr(v, "__len__") else v) for name, v in ((name, getattr(s, name)) for name, _ in s._fields_)}


def n_tiles(w, h):
    return ((w + A.FTN_METRICS_TILE - 1) // A.FTN_METRICS_TILE) * ((h + A.FTN_METRICS_TILE - 1) // A.FTN_METRICS_TILE)


def _compare(be, call, test, ref, params, error_map, ssim_map, tile_sums, totals):
    p = _params(be, params)
    test = host_image(test, 3)
    ref = host_image(ref, 3, test.shape[:2])
    h, w = test.shape[:2]
    res, tot = A.ftn_metrics_result(), A.ftn_metrics_totals()
    err = np.empty((h, w), np.float32) if error_map else None
    ssm = np.empty((h, w), np.float32) if ssim_map else None
    tiles = np.empty((n_tiles(w, h), A.FTN_METRICS_SUMS), np.float64) if tile_sums else None
    be.check(call(ptr(test), ptr(ref), w, h, C.byref(p), C.byref(res), C.byref(tot), ptr(err), ptr(ssm), ptr(tiles)))
    out = _struct_dict(res)
    for name, v, asked in (("error_map", err, error_map), ("ssim_map", ssm, ssim_map), ("tile_sums", tiles, tile_sums), ("totals", _struct_dict(tot), totals)):
        if asked:
            out[name] = v
    return out


def compare(be, test, ref, params=None, device=-1, error_map=False, ssim_map=False, tile_sums=False, totals=False):
    """ftn_metrics: the measures of `test` against `ref`, two host images, computed on GPU `device`."""
    fn = _lib(be).ftn_metrics
    return _compare(be, lambda *a: fn(*a, device), test, ref, params, error_map, ssim_map, tile_sums, totals)


def compare_cpu(be, test, ref, params=None, error_map=False, ssim_map=False, tile_sums=False, totals=False):
    """ftn_metrics_cpu: the host twin (the same bits)."""
    return _compare(be, _lib(be).ftn_metrics_cpu, test, ref, params, error_map, ssim_map, tile_sums, totals)


def workspace_size(be, w, h, flags=0):
    """ftn_metrics_workspace_size: bytes of device workspace for a w x h image."""
    n = C.c_size_t(0)
    be.check(_lib(be).ftn_metrics_workspace_size(w, h, flags, C.byref(n)))
    return n.value


def ssim_weights(be):
    """ftn_metrics_ssim_weights: g_0 .. g_10 as the kernels and the twin use them."""
    g = np.empty(A.FTN_METRICS_SSIM_TAPS, np.float64)
    be.check(_lib(be).ftn_metrics_ssim_weights(ptr(g)))
    return g


def resolve(be, totals, params=None):
    """ftn_metrics_resolve: the dict of ftn_metrics_result from an A.ftn_metrics_totals (or the 112 bytes of one)."""
    if not isinstance(totals, A.ftn_metrics_totals):
        totals = A.ftn_metrics_totals.from_buffer_copy(bytes(totals))
    p = _params(be, params)
    res = A.ftn_metrics_result()
    be.check(_lib(be).ftn_metrics_resolve(C.byref(totals), C.byref(p), C.byref(res)))
    return _struct_dict(res)


def compare_device(be, test_ptr, ref_ptr, w, h, totals_ptr, workspace_ptr, stream=0, params=None, error_map_ptr=0, ssim_map_ptr=0, tile_sums_ptr=0):
    """ftn_metrics_device: device pointers (test, ref: 3 w h floats; totals: an ftn_metrics_totals; the maps: w h floats; tile_sums:
    8 n_tiles doubles; workspace: workspace_size bytes), all 16-byte aligned, on `stream`.  The optional ones may be 0 or None."""
    p = _params(be, params)
    be.check(_lib(be).ftn_metrics_device(C.c_void_p(test_ptr), C.c_void_p(ref_ptr), w, h, C.byref(p), C.c_void_p(totals_ptr or None),
                                         C.c_void_p(error_map_ptr or None), C.c_void_p(ssim_map_ptr or None), C.c_void_p(tile_sums_ptr or None),
                                         C.c_void_p(workspace_ptr or None), C.c_void_p(stream)))


# ------------------------------------------------------------------ the command lines
THRESHOLD_NAMES = ("mse", "rmse", "mae", "rel_mse", "smape", "max_abs", "n_different", "n_nonfinite")


def report_line(r, ssim):
    """The line both command lines print for a comparison."""
    s = "rmse %.6g  mse %.6g  mae %.6g  rel_mse %.6g  smape %.6g  psnr %.4f dB  max_abs %.6g at pixel %d" % (
        r["rmse"], r["mse"], r["mae"], r["rel_mse"], r["smape"], r["psnr"], r["max_abs"], r["max_abs_index"])
    if ssim:
        s += "  ssim %.6f (%d windows)" % (r["ssim"], r["n_ssim_windows"])
    return s + "  %d of %d pixels differ, %d not finite" % (r["n_different"], r["n_pixels"], r["n_nonfinite"])


def exr_size(path, be):
    """(w, h) of an OpenEXR file: ftn_exr_read with a null buffer; None where it cannot be read."""
    w, h = C.c_uint32(), C.c_uint32()
    if be.lib.ftn_exr_read(os.fsencode(path), C.byref(w), C.byref(h), None) != 0:
        return None
    return w.value, h.value


def parse_thresholds(items):
    """--fail-above's NAME=VALUE items as a dict; ValueError with the usage message otherwise."""
    out = {}
    for item in items or ():
        name, eq, value = item.partition("=")
        try:
            v = float(value)
        except ValueError:
            v = float("nan")
        if not eq or name not in THRESHOLD_NAMES or math.isnan(v):
            raise ValueError("--fail-above takes NAME=VALUE with NAME one of %s" % ", ".join(THRESHOLD_NAMES))
        out[name] = v
    return out


def exceeded(r, thresholds):
    """The names of `thresholds` whose metric is above its value, or NaN."""
    return [name for name, v in thresholds.items() if not float(r[name]) <= v]


def main(argv=None):
    from .api import FountainError, read_exr, write_exr
    ap = argparse.ArgumentParser(prog="fountain_amd.metrics")
    ap.add_argument("test", help="the OpenEXR file to measure")
    ap.add_argument("ref", help="the OpenEXR file it is measured against")
    ap.add_argument("--ssim", action="store_true", help="compute SSIM as well (images of at least 11 x 11 pixels)")
    ap.add_argument("--peak", type=float, default=None, metavar="P", help="the signal's peak for PSNR and SSIM (default 1)")
    ap.add_argument("--rel-eps", type=float, default=None, metavar="E", help="the epsilon of relMSE and SMAPE (default 0.01)")
    ap.add_argument("--error-map", default=None, metavar="F.exr", help="write the per-pixel squared error (the mean of the channels)")
    ap.add_argument("--ssim-map", default=None, metavar="F.exr", help="write the per-pixel SSIM (needs --ssim)")
    ap.add_argument("--tile-map", default=None, metavar="F.exr", help="write the per-tile MSE, one pixel per 16 x 16 tile")
    ap.add_argument("--json", action="store_true", help="print the result as one JSON object")
    ap.add_argument("--cpu", action="store_true", help="run the host twin (the same bits; needs no GPU)")
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--fail-above", action="append", default=None, metavar="NAME=VALUE", help="exit with 1 when the metric exceeds the value or is NaN")
    opts = ap.parse_args(argv)
    try:
        thresholds = parse_thresholds(opts.fail_above)
    except ValueError as e:
        return refuse(e)
    for name, v in (("--error-map", opts.error_map), ("--ssim-map", opts.ssim_map), ("--tile-map", opts.tile_map)):
        if v is not None and not v.endswith(".exr"):
            return refuse("%s must name an .exr file" % name)
    if opts.ssim_map and not opts.ssim:
        return refuse("--ssim-map belongs to --ssim")
    for name, v in (("--peak", opts.peak), ("--rel-eps", opts.rel_eps)):
        if v is not None and not 0.0 < v < float("inf"):
            return refuse("%s takes a finite value above 0" % name)
    be = default_backend()
    sizes = [exr_size(path, be) for path in (opts.test, opts.ref)]
    for path, size in zip((opts.test, opts.ref), sizes):
        if size is None:
            return refuse("%s is not a readable OpenEXR file" % path)
    if sizes[0] != sizes[1]:
        return refuse("the images differ in size: %d x %d against %d x %d" % (sizes[0] + sizes[1]))
    if opts.ssim and min(sizes[0]) < A.FTN_METRICS_SSIM_TAPS:
        return refuse("--ssim needs images of at least 11 x 11 pixels")
    fields = {k: v for k, v in (("peak", opts.peak), ("rel_eps", opts.rel_eps)) if v is not None}
    p = MetricsParams(be, ssim=opts.ssim, **fields)
    test, ref = read_exr(opts.test, be), read_exr(opts.ref, be)
    want = dict(error_map=opts.error_map is not None, ssim_map=opts.ssim_map is not None, tile_sums=opts.tile_map is not None)
    try:
        r = compare_cpu(be, test, ref, p, **want) if opts.cpu else compare(be, test, ref, p, device=opts.gpu, **want)
    except FountainError as e:
        return refuse(e)
    w, h = sizes[0]
    grey = lambda plane: np.repeat(np.asarray(plane, np.float32)[:, :, None], 3, axis=2)
    if opts.error_map:
        write_exr(opts.error_map, grey(r.pop("error_map")), be)
    if opts.ssim_map:
        write_exr(opts.ssim_map, grey(r.pop("ssim_map")), be)
    if opts.tile_map:
        write_exr(opts.tile_map, grey(tile_mse(r.pop("tile_sums"), w, h)), be)
    over = exceeded(r, thresholds)
    if opts.json:
        print(json.dumps(dict(r, test=opts.test, ref=opts.ref, ssim_computed=bool(opts.ssim), exceeded=over)))
    else:
        print("metrics: " + report_line(r, opts.ssim))
    for name in over:
        print("metrics: %s = %.9g exceeds %.9g" % (name, r[name], thresholds[name]), file=sys.stderr)
    return 1 if over else 0


def tile_mse(tile_sums, w, h):
    """The per-tile MSE [ceil(h / 16), ceil(w / 16)] of compare's tile_sums: SE over three times the tile's pixels (bad ones included:
    the tile sums carry no count of their own)."""
    T = A.FTN_METRICS_TILE
    ty, tx = (h + T - 1) // T, (w + T - 1) // T
    rows = np.minimum(T, h - T * np.arange(ty))[:, None]
    cols = np.minimum(T, w - T * np.arange(tx))[None, :]
    return np.asarray(tile_sums)[:, 0].reshape(ty, tx) / (3.0 * rows * cols)


if __name__ == "__main__":
    sys.exit(main())
