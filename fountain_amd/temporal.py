"""Temporal reprojection and accumulation (include/fountain_hip_temporal.h) for frames of one static scene under a moving camera -- or,
with each frame's previous positions (`motion=`, include/fountain_hip_motion.h, fountain_amd/motion.py), of a scene whose objects move: each
frame's resolved beauty, resolved G-buffer (fountain_amd/gbuffer.py) and variance of the mean (fountain_amd/moments.py) are blended with
the history of the frames before it, fetched where the previous camera saw the pixel's surface.  The accumulated image and variance go
into the variance-guided filter (fountain_amd/denoise.py) unchanged.

  temporal_params(be, **fields)                                          ftn_temporal_params_default, then the given fields
  temporal_accumulate(be, rgb, gb12, var4, camera, film, prev=None, params=None, device=-1)   host arrays, accumulated on the GPU
  temporal_accumulate_cpu(be, rgb, gb12, var4, camera, film, prev=None, params=None)          the host twin, bit-identical to the GPU
  temporal_accumulate_torch(be, rgb, gb12, var4, camera, film, out_history, out_rgb, out_var4, prev=None, params=None)
                                                                         float32 CUDA tensors on the current stream, caller buffers
  TemporalAccumulator(be).push(rgb, gb12, var4, camera, film)            keeps the history and the previous frame between calls

rgb is [H, W, 3], gb12 [H, W, 12], var4 [H, W, 4]; history is [H, W, 8] (ftn_temporal_pixel: u r, g, b, the history length n, then the
variances of u in r, g, b and of Y).  `camera` has a .desc (PerspectiveCamera, or a PbrtScene's camera), `film` is the Film the frame
was rendered on (its crop is H x W).  `prev` is None for the first frame, else (previous camera, previous gb12, previous history).  Every
call and push() take `motion=None`: the frame's mv8 [H, W, 8] (motion.render_motion against the previous frame's scene), with which the
history is fetched where the pixel's surface point was in the previous frame and tested against where it stood; None is the static scene.  The
host calls return (history, rgb, var4) as new arrays.  The reference renders single frames, so the CPU oracle has no twin of these calls.

`python -m fountain_amd.temporal f0.pbrt f1.pbrt ... -o out.exr --samples N [--alpha-min A] [--denoise-guided]` renders the files as
successive frames of one static scene (the first file's; every file gives its frame's camera), frame k with sampler seed k, and writes
out_<k>.exr (the frame alone), out_<k>_accumulated.exr and, with --denoise-guided, out_<k>_denoised_guided.exr: the variance-guided filter
over the accumulated image and variance.  It needs at least 2 samples per pixel and files whose films agree.
With --dynamic every file's own scene is rendered (two scenes are alive at a time): frame k >= 1 renders its previous positions against
frame k - 1's scene, accumulates through them and also writes out_<k>_motion.exr, the screen-space motion in R and G (B = 0).  The files'
scenes must correspond (fountain_amd/motion.py); files that do not end with exit code 2 before anything is rendered or written.
With --dynamic --vector-blur [SHUTTER] frame k >= 1 also writes out_<k>_blurred.exr: the frame's own render blurred along its motion
vectors, with its G-buffer's depths (fountain_amd/vectorblur.py; the shutter is the share of the frame interval it is open, default 0.5).
"""
import ctypes as C
import sys

import numpy as np

from . import _abi as A
from ._cli import beside, refuse
from ._nontwin import bind, check_tensor, current_stream, desc_of as _desc, host_image, params_of, ptr, tptr


def _lib(be):
    return bind(be, A.EXTENSIONS["temporal"])


def _params(be, params):
    return params_of(be, params, A.ftn_temporal_params, "ftn_temporal_params_default", _lib, hidden=("reserved",))


def temporal_params(be, **fields):
    """ftn_temporal_params_default, then the given fields."""
    return _params(be, fields)


def _prev(prev):
    if prev is None:
        return None
    if not isinstance(prev, (tuple, list)) or len(prev) != 3 or any(x is None for x in prev):
        raise ValueError("prev must be None (the first frame) or (previous camera, previous gb12, previous history)")
    return prev


def _host_frame(rgb, gb12, var4, prev):
    try:
        rgb = host_image(rgb, 3)
        gb12, var4 = host_image(gb12, 12, rgb.shape[:2]), host_image(var4, 4, rgb.shape[:2])
    except ValueError:
        raise ValueError("expected rgb [H, W, 3], gb12 [H, W, 12] and var4 [H, W, 4], got %r, %r and %r"
                         % (np.shape(rgb), np.shape(gb12), np.shape(var4))) from None
    prev = _prev(prev)
    if prev is not None:
        try:
            pgb, ph = host_image(prev[1], 12, rgb.shape[:2]), host_image(prev[2], 8, rgb.shape[:2])
        except ValueError:
            raise ValueError("expected a previous gb12 %r and a previous history %r, got %r and %r"
                             % (gb12.shape, rgb.shape[:2] + (8,), np.shape(prev[1]), np.shape(prev[2]))) from None
        prev = (_desc(prev[0], A.ftn_camera_desc, "the previous camera"), pgb, ph)
    return rgb, gb12, var4, prev


def _motion_lib(be):
    return bind(be, A.EXTENSIONS["motion"])


def _host_call(be, fn, rgb, gb12, var4, camera, film, prev, params, tail, motion=None):
    p = _params(be, params)
    cam, fd = _desc(camera, A.ftn_camera_desc, "camera"), _desc(film, A.ftn_film_desc, "film")
    rgb, gb12, var4, prev = _host_frame(rgb, gb12, var4, prev)
    h, w = rgb.shape[:2]
    hist, out, ovar = np.empty((h, w, 8), np.float32), np.empty_like(rgb), np.empty_like(var4)
    pc, pg, ph = (C.byref(prev[0]), ptr(prev[1]), ptr(prev[2])) if prev is not None else (None, None, None)
    if motion is None:
        be.check(fn(ptr(rgb), ptr(gb12), ptr(var4), C.byref(cam), C.byref(fd), w, h, pc, pg, ph, C.byref(p), ptr(hist), ptr(out), ptr(ovar), *tail))
        return hist, out, ovar
    try:
        mv8 = host_image(motion, 8, rgb.shape[:2])
    except ValueError:
        raise ValueError("expected motion (mv8) %r, got %r" % (rgb.shape[:2] + (8,), np.shape(motion))) from None
    fn = getattr(_motion_lib(be), fn.__name__.replace("ftn_temporal_accumulate", "ftn_temporal_accumulate_motion"))
    be.check(fn(ptr(rgb), ptr(gb12), ptr(var4), ptr(mv8), C.byref(cam), C.byref(fd), w, h, pc, pg, ph, C.byref(p), ptr(hist), ptr(out), ptr(ovar), *tail))
    return hist, out, ovar


def temporal_accumulate(be, rgb, gb12, var4, camera, film, prev=None, params=None, device=-1, motion=None):
    """ftn_temporal_accumulate (with `motion`, the frame's mv8: ftn_temporal_accumulate_motion): host arrays, accumulated on GPU `device`
    (-1 = the current one); returns (history, rgb, var4)."""
    return _host_call(be, _lib(be).ftn_temporal_accumulate, rgb, gb12, var4, camera, film, prev, params, (device,), motion)


def temporal_accumulate_cpu(be, rgb, gb12, var4, camera, film, prev=None, params=None, motion=None):
    """ftn_temporal_accumulate_cpu (with `motion`: ftn_temporal_accumulate_motion_cpu): the host twin (same bits as the GPU); returns
    (history, rgb, var4)."""
    return _host_call(be, _lib(be).ftn_temporal_accumulate_cpu, rgb, gb12, var4, camera, film, prev, params, (), motion)


def temporal_accumulate_torch(be, rgb, gb12, var4, camera, film, out_history, out_rgb, out_var4, prev=None, params=None, motion=None):
    """ftn_temporal_accumulate_device: rgb [H, W, 3], gb12 [H, W, 12], var4 [H, W, 4] -> out_history [H, W, 8], out_rgb [H, W, 3] and
    out_var4 [H, W, 4], contiguous float32 CUDA tensors on one device, on its current stream; prev = (previous camera, previous gb12
    tensor, previous history tensor) or None; motion = the frame's mv8 tensor [H, W, 8] or None (ftn_temporal_accumulate_motion_device with
    it).  The call allocates nothing, so it can be captured in a graph.  Returns (out_history,
    out_rgb, out_var4)."""
    import torch
    lib = _lib(be)
    p = _params(be, params)
    cam, fd = _desc(camera, A.ftn_camera_desc, "camera"), _desc(film, A.ftn_film_desc, "film")
    if not isinstance(rgb, torch.Tensor) or rgb.dim() != 3:
        raise ValueError("expected a contiguous float32 CUDA tensor rgb [H, W, 3]")
    h, w = rgb.shape[:2]
    prev = _prev(prev)
    tensors = [(rgb, 3), (gb12, 12), (var4, 4), (out_history, 8), (out_rgb, 3), (out_var4, 4)] + ([(prev[1], 12), (prev[2], 8)] if prev is not None else [])
    if motion is not None:
        tensors.append((motion, 8))
    for t, k in tensors:
        check_tensor(t, (h, w, k))
        if t.device != rgb.device:
            raise ValueError("every tensor must live on the device of rgb")
    pc, pg, ph = (C.byref(_desc(prev[0], A.ftn_camera_desc, "the previous camera")), tptr(prev[1]), tptr(prev[2])) \
        if prev is not None else (None, None, None)
    dp = lambda t: tptr(t)
    rest = (C.byref(cam), C.byref(fd), w, h, pc, pg, ph, C.byref(p), tptr(out_history), tptr(out_rgb), tptr(out_var4), C.c_void_p(current_stream(rgb)))
    if motion is not None:
        be.check(_motion_lib(be).ftn_temporal_accumulate_motion_device(tptr(rgb), tptr(gb12), tptr(var4), tptr(motion), *rest))
    else:
        be.check(lib.ftn_temporal_accumulate_device(tptr(rgb), tptr(gb12), tptr(var4), *rest))
    return out_history, out_rgb, out_var4


class TemporalAccumulator:
    """The state a frame sequence carries: the history, the previous frame's G-buffer and its camera.  push() accumulates one frame on
    the GPU (on the host twin with cpu=True) and returns (accumulated rgb, accumulated var4) -- with `motion`, the frame's mv8 against the
    previous frame's scene, through ftn_temporal_accumulate_motion (a first frame has no previous frame and ignores it); reset() forgets the history, so the next
    frame is a first frame.  A frame of another size resets by itself."""

    def __init__(self, be, params=None, device=-1, cpu=False):
        self.be, self.device, self.cpu = be, device, cpu
        self.params = _params(be, params)
        self.reset()

    def reset(self):
        self.history = None             # [H, W, 8] after the first push
        self.prev_gb12 = None
        self.prev_camera = None
        self.frames = 0

    def push(self, rgb, gb12, var4, camera, film, motion=None):
        cam = _desc(camera, A.ftn_camera_desc, "camera")
        if self.history is not None and self.history.shape[:2] != np.shape(rgb)[:2]:
            self.reset()
        prev = None if self.history is None else (self.prev_camera, self.prev_gb12, self.history)
        if self.cpu:
            hist, out, ovar = temporal_accumulate_cpu(self.be, rgb, gb12, var4, cam, film, prev, self.params, motion=motion)
        else:
            hist, out, ovar = temporal_accumulate(self.be, rgb, gb12, var4, cam, film, prev, self.params, self.device, motion=motion)
        keep = A.ftn_camera_desc()
        C.memmove(C.byref(keep), C.byref(cam), C.sizeof(cam))
        self.history, self.prev_gb12, self.prev_camera = hist, np.array(gb12, dtype=np.float32), keep
        self.frames += 1
        return out, ovar


def motion_path(filename, k):
    """out.exr, k -> out_<k>_motion.exr (--dynamic)"""
    return beside(filename, "_%d_motion.exr" % k)


def blurred_path(filename, k):
    """out.exr, k -> out_<k>_blurred.exr (--dynamic --vector-blur)"""
    return beside(filename, "_%d_blurred.exr" % k)


def frame_paths(filename, k):
    """out.exr, k -> (out_<k>.exr, out_<k>_accumulated.exr, out_<k>_denoised_guided.exr)"""
    return tuple(beside(filename, "_%d%s.exr" % (k, s)) for s in ("", "_accumulated", "_denoised_guided"))


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="fountain_amd.temporal")
    ap.add_argument("scene_files", nargs="+", help="one .pbrt file per frame: the first one's scene, every file's camera")
    ap.add_argument("-o", "--output", dest="image_name", default=None)
    ap.add_argument("--samples", type=int, default=None)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--max-depth", type=int, default=5)
    ap.add_argument("--rr-threshold", type=float, default=1.0)
    ap.add_argument("--alpha-min", type=float, default=None, help="floor of the current frame's blend weight, 0..1 (default: the library's)")
    ap.add_argument("--denoise-guided", action="store_true",
                    help="also write <name>_<k>_denoised_guided.exr: the variance-guided filter over the accumulated image and variance")
    ap.add_argument("--dynamic", action="store_true",
                    help="every file's own scene: objects may move between frames (the files' scenes must correspond); frame k >= 1 follows "
                         "them through its previous positions and also writes <name>_<k>_motion.exr")
    ap.add_argument("--vector-blur", type=float, nargs="?", const=True, default=None, metavar="SHUTTER",
                    help="with --dynamic: also write <name>_<k>_blurred.exr, frame k >= 1 blurred along its motion vectors; the shutter is open "
                         "for this share of the frame interval, 0..1 (default 0.5)")
    opts = ap.parse_args(argv)
    if opts.vector_blur is not None and not opts.dynamic:
        return refuse("--vector-blur belongs to --dynamic: a static scene's frames carry no motion vectors")
    if opts.vector_blur is not None and opts.vector_blur is not True and not 0.0 <= opts.vector_blur <= 1.0:
        return refuse("--vector-blur takes a shutter in [0, 1]")
    if opts.dynamic and len(opts.scene_files) < 2:
        return refuse("--dynamic needs at least two frames: a frame's motion is against the frame before it")
    if opts.samples is not None and opts.samples < 2:
        return refuse("temporal accumulation needs at least 2 samples per pixel: a pixel's variance is unknown below that (here %d)" % opts.samples)
    if opts.alpha_min is not None and not 0.0 <= opts.alpha_min <= 1.0:
        return refuse("--alpha-min must be in 0..1")
    from .api import PathIntegrator, PbrtScene, RandomSampler, default_backend, write_exr
    from .denoise import denoise_guided
    from .gbuffer import CHANNELS, render_gbuffer
    from .moments import render_moments
    be = default_backend()
    frames = [PbrtScene(f, be) for f in opts.scene_files]
    first = frames[0]
    spp = opts.samples or first.samples_per_pixel
    if spp < 2:
        return refuse("temporal accumulation needs at least 2 samples per pixel: a pixel's variance is unknown below that (here %d)" % spp)
    for f, name in zip(frames[1:], opts.scene_files[1:]):
        if bytes(f._film_desc) != bytes(first._film_desc):
            return refuse("%s has another film than %s: the frames of a sequence share resolution and crop" % (name, opts.scene_files[0]))
    filename = opts.image_name or first.film_name
    if ".exr" not in filename:
        raise SystemExit("output must be an .exr file")
    if opts.dynamic:
        from .motion import descs_differ, motion_vectors, render_motion
        for k in range(1, len(frames)):
            why = descs_differ(frames[k].desc, frames[k - 1].desc)
            if why:
                return refuse("--dynamic: the scenes of %s and %s do not correspond: %s" % (opts.scene_files[k], opts.scene_files[k - 1], why))
    scene = first.create_scene(device=opts.gpu)
    prev_scene = None
    radiance = PathIntegrator.new(opts.max_depth, opts.rr_threshold)
    acc = TemporalAccumulator(be, None if opts.alpha_min is None else dict(alpha_min=opts.alpha_min), device=opts.gpu)
    for k, f in enumerate(frames):
        sampler = RandomSampler.new_with_seed(spp, k, indexed=True)
        if opts.dynamic and k > 0:       # this file's own scene; the one before it stays for the pass, the one before that is destroyed
            prev_scene = scene
            scene = f.create_scene(device=opts.gpu)
        var4, film, _, _ = render_moments(be, None, f.camera, None, radiance, sampler, scene=scene, film=f.film(), device=opts.gpu)
        img, _ = film.into_spectrum_buffer()
        res, _, _ = render_gbuffer(be, None, f.camera, None, sampler, scene=scene, film=f.film(), device=opts.gpu)
        gb12 = np.concatenate([res[c] for c in CHANNELS], axis=-1)
        mv8 = None
        if prev_scene is not None:
            prev_camera = acc.prev_camera
            mv8, _, _ = render_motion(be, None, f.camera, None, sampler, scene=scene, prev_scene=prev_scene, film=f.film(), device=opts.gpu)
        out, ovar = acc.push(img, gb12, var4, f.camera, film, motion=mv8)
        plain, accumulated, denoised = frame_paths(filename, k)
        if mv8 is not None:
            mv = motion_vectors(be, mv8, gb12, f.camera, prev_camera, film, device=opts.gpu)
            write_exr(motion_path(filename, k), np.concatenate([mv, np.zeros_like(mv[..., :1])], axis=-1), be)
            if opts.vector_blur is not None:
                from .vectorblur import vector_blur
                shutter = {} if opts.vector_blur is True else dict(shutter=opts.vector_blur)
                write_exr(blurred_path(filename, k), vector_blur(be, img, mv, gb12, shutter, device=opts.gpu), be)
        write_exr(plain, img, be)
        write_exr(accumulated, out, be)
        if opts.denoise_guided:
            write_exr(denoised, denoise_guided(be, out, gb12, ovar, device=opts.gpu), be)
        print("frame %d: %s, %s%s (mean history length %.2f)" % (k, plain, accumulated, ", " + denoised if opts.denoise_guided else "",
                                                                  float(acc.history[..., 3].mean())), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
