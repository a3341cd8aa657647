"""The vector-blur stage (include/fountain_hip_vectorblur.h): motion blur of a resolved image along the screen-space motion vectors of
fountain_amd/motion.py -- half velocities per pixel, the longest per 16 x 16 tile and per 3 x 3 tiles, and a gather along that direction
whose weights compare depths and velocities, so that a sharp foreground stays sharp over a moving background.

  VectorBlurParams(be=None, **fields)                                  .desc is an ftn_vectorblur_params
  vector_blur(be, rgb, motion, gb12=None, params=None, device=-1)      -> float32 [H, W, 3], computed on the GPU
  vector_blur_cpu(be, rgb, motion, gb12=None, params=None)             the host twin, bit-identical to the GPU
  velocities_cpu(be, motion, gb12=None, params=None)                   the host twin's steps 1 to 3: split_workspace's dict
  workspace_size(be, w, h)                                             -> bytes of device workspace vector_blur_device needs
  split_workspace(ws, w, h)                                            a workspace's floats as dict(pixels [H, W, 4], tiles and
                                                                       neighbours [tiles_y, tiles_x, 4])
  vector_blur_device(be, rgb, motion, gb12, out_rgb, workspace, stream=None, params=None)
      contiguous CUDA tensors on one device, on `stream` (a torch stream; None = the current one); allocates nothing, does not
      synchronise, launches kernels only

`params` is a VectorBlurParams, an A.ftn_vectorblur_params, a dict of VectorBlurParams' arguments, or None for the defaults.  rgb is
[H, W, 3] float32 (ftn_film_resolve), motion [H, W, 2] (motion.motion_vectors: previous minus current raster position, NaN = unknown), gb12
[H, W, 12] or None (every pixel at one depth).  The reference renders single frames without a shutter, so the CPU oracle has no twin of
these calls.

  python -m fountain_amd.vectorblur in.exr --motion in_motion.exr [--depth in_depth.exr] [--shutter S] [--taps N] [--max-radius R] -o out.exr
blurs an existing OpenEXR file along the R and G channels of the motion file (what fountain_amd.temporal --dynamic writes); the depth file
is camera-space depth in R (what fountain_amd.render --gbuffer writes), a pixel whose depth is not finite or not above 0 being background.
"""
import argparse
import ctypes as C
import sys

import numpy as np

from . import _abi as A
from ._cli import beside, refuse
from ._nontwin import bind, check_tensor, check_workspace, host_image, params_of, ptr, set_fields, tptr
from .api import default_backend

TILE = A.FTN_VECTORBLUR_MAX_RADIUS


def _lib(be):
    return bind(be, A.EXTENSIONS["vectorblur"])


class VectorBlurParams:
    def __init__(self, be=None, **fields):
        """ftn_vectorblur_params_default, then any other field of ftn_vectorblur_params (taps, shutter, max_radius, depth_extent)."""
        self.be = be or default_backend()
        self.desc = A.ftn_vectorblur_params()
        _lib(self.be).ftn_vectorblur_params_default(C.byref(self.desc))
        set_fields(self.desc, fields, hidden=("reserved",))


def _params(be, params):
    return params_of(be, params, A.ftn_vectorblur_params, "ftn_vectorblur_params_default", _lib, VectorBlurParams)


def _motion(motion, hw=None):
    m = np.ascontiguousarray(motion, dtype=np.float32)
    if m.ndim != 3 or m.shape[-1] != 2 or (hw is not None and m.shape[:2] != tuple(hw)):
        raise ValueError("expected motion [H, W, 2]%s, got %r" % (" with H, W = %r" % (tuple(hw),) if hw is not None else "", m.shape))
    return m


def _host_inputs(rgb, motion, gb12):
    rgb = host_image(rgb, 3)
    return rgb, _motion(motion, rgb.shape[:2]), None if gb12 is None else host_image(gb12, 12, rgb.shape[:2])


def vector_blur(be, rgb, motion, gb12=None, params=None, device=-1):
    """ftn_vectorblur: the blurred image of host arrays, computed on GPU `device`."""
    p = _params(be, params)
    rgb, motion, gb12 = _host_inputs(rgb, motion, gb12)
    out = np.empty_like(rgb)
    be.check(_lib(be).ftn_vectorblur(ptr(rgb), ptr(motion), ptr(gb12), rgb.shape[1], rgb.shape[0], C.byref(p), ptr(out), device))
    return out


def vector_blur_cpu(be, rgb, motion, gb12=None, params=None):
    """ftn_vectorblur_cpu: the host twin (the same bits)."""
    p = _params(be, params)
    rgb, motion, gb12 = _host_inputs(rgb, motion, gb12)
    out = np.empty_like(rgb)
    be.check(_lib(be).ftn_vectorblur_cpu(ptr(rgb), ptr(motion), ptr(gb12), rgb.shape[1], rgb.shape[0], C.byref(p), ptr(out)))
    return out


def workspace_size(be, w, h):
    """ftn_vectorblur_workspace_size: bytes of device workspace for a w x h image."""
    n = C.c_size_t(0)
    be.check(_lib(be).ftn_vectorblur_workspace_size(w, h, C.byref(n)))
    return n.value


def split_workspace(ws, w, h):
    """The float32 words of a workspace (a flat array of at least workspace_size / 4 floats) as the header lays them out: the pixels'
    records {h.x, h.y, len, z}, the tiles' and the neighbours' records {h.x, h.y, key, 0}."""
    ws = np.asarray(ws, dtype=np.float32).reshape(-1)
    tx, ty = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
    a, b = 4 * w * h, 4 * w * h + 4 * tx * ty
    return dict(pixels=ws[:a].reshape(h, w, 4), tiles=ws[a:b].reshape(ty, tx, 4), neighbours=ws[b:b + 4 * tx * ty].reshape(ty, tx, 4))


def velocities_cpu(be, motion, gb12=None, params=None):
    """ftn_vectorblur_velocities_cpu: steps 1 to 3 of the host twin, the bits vector_blur_device leaves in its workspace."""
    p = _params(be, params)
    motion = _motion(motion)
    h, w = motion.shape[:2]
    gb12 = None if gb12 is None else host_image(gb12, 12, (h, w))
    ws = np.empty(workspace_size(be, w, h) // 4, np.float32)
    be.check(_lib(be).ftn_vectorblur_velocities_cpu(ptr(motion), ptr(gb12), w, h, C.byref(p), ptr(ws)))
    return split_workspace(ws, w, h)


def vector_blur_device(be, rgb, motion, gb12, out_rgb, workspace, stream=None, params=None):
    """ftn_vectorblur_device: rgb and out_rgb [H, W, 3], motion [H, W, 2] and gb12 [H, W, 12] or None, contiguous float32 CUDA tensors on one
    device; workspace a contiguous CUDA tensor of at least workspace_size bytes there.  Returns out_rgb."""
    import torch
    p = _params(be, params)
    if not isinstance(rgb, torch.Tensor) or rgb.dim() != 3:
        raise ValueError("expected a contiguous float32 CUDA tensor rgb [H, W, 3]")
    h, w = rgb.shape[:2]
    for t, k in [(rgb, 3), (motion, 2), (out_rgb, 3)] + ([(gb12, 12)] if gb12 is not None else []):
        check_tensor(t, (h, w, k))
        if t.device != rgb.device:
            raise ValueError("every tensor must live on the device of rgb")
    check_workspace(workspace, workspace_size(be, w, h), rgb.device)
    s = (torch.cuda.current_stream(rgb.device) if stream is None else stream).cuda_stream
    be.check(_lib(be).ftn_vectorblur_device(tptr(rgb), tptr(motion), tptr(gb12), w, h, C.byref(p), tptr(out_rgb), tptr(workspace), C.c_void_p(s)))
    return out_rgb


def value_refusal(shutter=None, taps=None, max_radius=None):
    """What is wrong with the values of the command lines' options (the ranges of include/fountain_hip_vectorblur.h), or None."""
    if shutter is not None and not 0.0 <= shutter <= 1.0:
        return "the shutter must be in [0, 1]"
    if taps is not None and not 1 <= taps <= A.FTN_VECTORBLUR_MAX_TAPS:
        return "--taps takes 1..%d" % A.FTN_VECTORBLUR_MAX_TAPS
    if max_radius is not None and not 0.0 < max_radius <= A.FTN_VECTORBLUR_MAX_RADIUS:
        return "--max-radius takes a value in (0, %d]: a blur stays within the tiles around its own" % A.FTN_VECTORBLUR_MAX_RADIUS
    return None


def gb12_from_depth(depth):
    """A G-buffer that carries only what the stage reads, from camera-space depth [H, W]: a depth that is not finite or not above 0 is
    background (coverage 0)."""
    depth = np.asarray(depth, dtype=np.float32)
    gb12 = np.zeros(depth.shape + (12,), np.float32)
    with np.errstate(invalid="ignore"):
        hit = np.isfinite(depth) & (depth > 0)
    gb12[..., 9] = np.where(hit, depth, 0)
    gb12[..., 10] = hit
    return gb12


def main(argv=None):
    from .api import read_exr, write_exr
    ap = argparse.ArgumentParser(prog="fountain_amd.vectorblur")
    ap.add_argument("image", help="a linear-light OpenEXR file")
    ap.add_argument("--motion", required=True, metavar="FILE", help="the motion vectors in R and G, in pixels (fountain_amd.temporal --dynamic: <name>_<k>_motion.exr)")
    ap.add_argument("--depth", default=None, metavar="FILE", help="camera-space depth in R (fountain_amd.render --gbuffer: <name>_depth.exr); default: one depth everywhere")
    ap.add_argument("-o", "--output", default=None, help="the blurred OpenEXR file (default: the input's name with _blurred.exr)")
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--shutter", type=float, default=None, metavar="S", help="the share of the frame interval the shutter is open, 0..1 (default 0.5)")
    ap.add_argument("--taps", type=int, default=None, metavar="N", help="taps per pixel, 1..64 (default 16)")
    ap.add_argument("--max-radius", type=float, default=None, metavar="R", help="the longest half blur in pixels, up to 16 (default 16)")
    opts = ap.parse_args(argv)
    out = opts.output or beside(opts.image, "_blurred.exr")
    if not out.endswith(".exr"):
        return refuse("the output must be an .exr file")
    why = value_refusal(opts.shutter, opts.taps, opts.max_radius)
    if why:
        return refuse(why)
    be = default_backend()
    p = VectorBlurParams(be, **{k: v for k, v in (("shutter", opts.shutter), ("taps", opts.taps), ("max_radius", opts.max_radius)) if v is not None})
    rgb = read_exr(opts.image, be)
    motion = read_exr(opts.motion, be)
    depth = read_exr(opts.depth, be) if opts.depth else None
    for name, a in ((opts.motion, motion), (opts.depth, depth)):
        if a is not None and a.shape != rgb.shape:
            return refuse("%s is %d x %d, %s is %d x %d" % (name, a.shape[1], a.shape[0], opts.image, rgb.shape[1], rgb.shape[0]))
    gb12 = None if depth is None else gb12_from_depth(depth[..., 0])
    write_exr(out, vector_blur(be, rgb, motion[..., :2], gb12, p, device=opts.gpu), be)
    print("vector blur: %s (shutter %.6g, %d taps)" % (out, p.desc.shutter, p.desc.taps), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
