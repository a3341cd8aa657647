"""The scaffold of the first-hit passes' bindings whose raw pixels are float sums (gbuffer.py, ao.py, motion.py, lightpass.py): each pass
describes itself in a FirstHitPass, and its public functions are thin calls of the four functions here.  What a pass's entries take
beyond the common arguments it hands over itself: `lead`, a tuple that follows the scene (motion's previous scene), and `extra`, a
function without arguments whose tuple goes between the options and the pixels (ao's options, the light list) -- a function, so that it
is evaluated where the pass's own code used to evaluate it: after the checks and call_args.  idmatte.py, the fifth first-hit pass, keeps
its calls written out: its tables are uint32 words, and it converts its ids between the raw buffer's check and call_args."""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _abi as A
from ._nontwin import bind, call_args, check_tensor, current_stream, ptr, tptr
from .api import Film

# ext: the A.Extension; words: floats of a raw pixel; resolved: floats of a resolved pixel; entries: the C names of host render, device
# render, host resolve, device resolve; channels: name -> slice of a resolved pixel.  The render functions read ext, words and the first
# two entries; `resolved` and the other two are for resolve_host / resolve_torch (gbuffer.py, whose resolves are written out, uses only
# `channels` of them).
FirstHitPass = namedtuple("FirstHitPass", "ext words resolved entries channels")


def _none():
    return ()


def render_host(p, be, builder, cam, res, sampler, *, tiles, crop, scene, raw, pipeline, device, film, count_traffic=False, lead=(), extra=_none):
    """create_scene (unless `scene` is given) + Film (unless `film` is given) + the pass's host render entry, added into `raw` (a zero
    buffer when None).  Returns (raw, stats)."""
    lib = bind(be, p.ext)
    scene = scene or builder.create_scene()
    film = film or Film(be, res, crop)
    shape = (film.height, film.width, p.words)
    if raw is None:
        raw = np.zeros(shape, np.float32)
    if raw.shape != shape or raw.dtype != np.float32 or not raw.flags.c_contiguous:
        raise ValueError("raw must be a C-contiguous float32 array of shape %r" % (shape,))
    args, keep = call_args(cam, film, None, sampler, tiles, pipeline, device, count_traffic)
    st = A.ftn_stats()
    be.check(getattr(lib, p.entries[0])(scene.handle, *lead, *args, *extra(), ptr(raw), C.byref(st)))
    return raw, st.as_dict()


def render_torch(p, scene, cam, film, sampler, out, *, tiles, pipeline, lead=(), extra=_none):
    """The pass's device render entry into `out` (float32 CUDA tensor [H, W, words], added into) on the current stream of its device.
    Returns the stats."""
    be = scene.be
    lib = bind(be, p.ext)
    check_tensor(out, (film.height, film.width, p.words))
    args, keep = call_args(cam, film, None, sampler, tiles, pipeline, out.device.index)
    st = A.ftn_stats()
    be.check(getattr(lib, p.entries[1])(scene.handle, *lead, *args, *extra(), tptr(out), C.c_void_p(current_stream(out)), C.byref(st)))
    return st.as_dict()


def resolve_host(p, be, raw, extra=_none):
    """The pass's host resolve entry: raw [..., words] sums -> a new array [..., resolved]."""
    lib = bind(be, p.ext)
    raw = np.ascontiguousarray(raw, dtype=np.float32)
    if raw.shape[-1] != p.words:
        raise ValueError("the last dimension holds the %d floats of a pixel" % p.words)
    out = np.empty(raw.shape[:-1] + (p.resolved,), np.float32)
    be.check(getattr(lib, p.entries[2])(ptr(raw), raw.size // p.words, *extra(), ptr(out)))
    return out


def resolve_torch(p, be, raw, out, extra=_none):
    """The pass's device resolve entry: raw [..., words] sums -> out [..., resolved], both float32 CUDA tensors, current stream."""
    lib = bind(be, p.ext)
    check_tensor(raw, raw.shape)
    if raw.shape[-1] != p.words:
        raise ValueError("the last dimension holds the %d floats of a pixel" % p.words)
    check_tensor(out, tuple(raw.shape[:-1]) + (p.resolved,))
    be.check(getattr(lib, p.entries[3])(tptr(raw), raw.numel() // p.words, *extra(), tptr(out), C.c_void_p(current_stream(raw))))
    return out


def channels(p, out):
    """A resolved array as the dict of the pass's channels."""
    return {k: out[..., s] for k, s in p.channels.items()}
