"""Light-group AOVs (include/fountain_hip_lightpass.h) over exactly the camera samples ftn_render traces for the same sampler, tiles and
film: per group of lights, the direct light that arrives at the first visible surface (`unshadowed`) and the part of it the scene lets
through (`lit`), one light sample and one shadow ray per surface through the production any-hit kernels.  A compositor scales and sums
the groups afterwards (compose) instead of rendering again.

  render_lightpass(be, builder, cam, res, sampler, lights=None)     host buffers -> (resolved dict of [H, W, k] arrays, raw [H, W, 8] sums, stats)
  render_lightpass_torch(scene, cam, film, sampler, out, lights)    adds into a float32 CUDA tensor [H, W, 8] on the current stream
  resolve(be, raw) / resolve_torch(be, raw, out)                    sums -> the 8 resolved floats per pixel
  compose(be, gb12, res8, gains) / compose_torch(...)               the relighting step: sum over groups of albedo / pi * lit * gain
  terms(be, hit24, light24, group_size)                             the term and the shadow ray of surfaces and light samples, on the host
  groups(scene, by="kind")                                          name -> index list, from ftn_scene_get_lights

`lights` is a strictly increasing list of indices into the scene's lights (Scene.lights() order), None for all of them.  The raw layout is
ftn_lightpass_pixel: lit 3, unshadowed 3, hit_weight, weight.  The reference has no light AOVs, so the CPU oracle has no twin of these
calls.

`python -m fountain_amd.lightpass relight --albedo A.exr --light G=FILE:r,g,b ... -o out.exr` runs compose on files: A.exr is the
G-buffer's albedo, every FILE a <name>_light_<group>.exr of `render.py --light-groups`, and r,g,b that group's gain.
"""
import ctypes as C
import sys

import numpy as np

from . import _abi as A, _firsthit as F
from ._cli import refuse
from ._nontwin import bind, check_tensor as _check_tensor, current_stream, host_image, index_list, ptr, tptr

# resolved channels: name -> slice of the 8 floats ftn_lightpass_resolve writes per pixel
CHANNELS = {"lit": slice(0, 3), "unshadowed": slice(3, 6), "visibility": slice(6, 7), "coverage": slice(7, 8)}
PASS = F.FirstHitPass(A.EXTENSIONS["lightpass"], 8, 8,
                      ("ftn_render_lightpass", "ftn_render_lightpass_device", "ftn_lightpass_resolve", "ftn_lightpass_resolve_device"), CHANNELS)
KINDS = ("point", "distant", "infinite", "area")          # ftn_scene_get_lights' kinds 0 .. 3


def _lib(be):
    return bind(be, PASS.ext)


def groups(scene, by="kind"):
    """The index lists of a scene's light groups, name -> list, in the order of Scene.lights().  by="kind": one group per kind that
    has lights (point, distant, infinite, area); by="each": light<i> for every explicit light, and `area` for the area lights together."""
    kind, _ = scene.lights()
    if by == "kind":
        out = {name: [i for i, k in enumerate(kind) if k == code] for code, name in enumerate(KINDS)}
    elif by == "each":
        out = {"light%d" % i: [i] for i, k in enumerate(kind) if k != 3}
        out["area"] = [i for i, k in enumerate(kind) if k == 3]
    else:
        raise ValueError("groups are made by 'kind' or by 'each'")
    return {name: idx for name, idx in out.items() if idx}


def resolve(be, raw):
    """ftn_lightpass_resolve: raw [H, W, 8] sums -> dict of resolved [H, W, k] arrays (CHANNELS)."""
    return F.channels(PASS, resolve8(be, raw))


def resolve8(be, raw):
    """ftn_lightpass_resolve: raw [..., 8] sums -> the resolved [..., 8] floats as one array (what compose takes)."""
    return F.resolve_host(PASS, be, raw)


def _gains(gains, n_groups):
    g = np.ascontiguousarray(gains, dtype=np.float32)
    if g.shape != (n_groups, 3):
        raise ValueError("one gain (r, g, b) per group: expected shape %r, got %r" % ((n_groups, 3), g.shape))
    return g


def compose(be, gb12, res8, gains):
    """ftn_lightpass_compose (the host twin of the kernel): gb12 [H, W, 12] resolved G-buffer, res8 [groups, H, W, 8] resolved light
    passes, gains [groups, 3] -> rgb [H, W, 3]."""
    lib = _lib(be)
    gb12 = host_image(gb12, 12)
    res8 = np.ascontiguousarray(res8, dtype=np.float32)
    if res8.ndim != 4 or res8.shape[1:] != gb12.shape[:2] + (8,):
        raise ValueError("expected res8 [groups, H, W, 8] with the G-buffer's H and W, got %r" % (res8.shape,))
    g = _gains(gains, res8.shape[0])
    out = np.empty(gb12.shape[:2] + (3,), np.float32)
    be.check(lib.ftn_lightpass_compose(ptr(gb12), ptr(res8), res8.shape[0], ptr(g), gb12.shape[0] * gb12.shape[1], ptr(out)))
    return out


def compose_torch(be, gb12, res8, gains, out):
    """ftn_lightpass_compose_device: float32 CUDA tensors gb12 [H, W, 12], res8 [groups, H, W, 8] -> out [H, W, 3], current stream; gains
    is a host array [groups, 3]."""
    lib = _lib(be)
    _check_tensor(gb12, tuple(gb12.shape[:2]) + (12,))
    _check_tensor(res8, (res8.shape[0],) + tuple(gb12.shape[:2]) + (8,))
    _check_tensor(out, tuple(gb12.shape[:2]) + (3,))
    g = _gains(gains, res8.shape[0])
    be.check(lib.ftn_lightpass_compose_device(tptr(gb12), tptr(res8), res8.shape[0], ptr(g),
                                              gb12.shape[0] * gb12.shape[1], tptr(out), C.c_void_p(current_stream(gb12))))
    return out


def terms(be, hit24, light24, group_size):
    """ftn_lightpass_terms: for n interaction records in ftn_intersect_full's layout ([n, 24]) and n output rows of the light hook
    ([n, 24]), the pass's term e [n, 3] and shadow ray [n, 8] = {o, d, t_max, 0} (zeros where no ray is traced).  Runs on the host."""
    lib = _lib(be)
    hit24 = np.ascontiguousarray(hit24, dtype=np.float32).reshape(-1, 24)
    light24 = np.ascontiguousarray(light24, dtype=np.float32).reshape(-1, 24)
    if len(hit24) != len(light24):
        raise ValueError("one light sample per interaction record")
    e, rays = np.empty((len(hit24), 3), np.float32), np.empty((len(hit24), 8), np.float32)
    be.check(lib.ftn_lightpass_terms(ptr(hit24), ptr(light24), len(hit24), int(group_size), ptr(e), ptr(rays)))
    return e, rays


def render_lightpass(be, builder, cam, res, sampler, lights=None, tiles=None, crop=(0.0, 0.0, 1.0, 1.0), scene=None, raw=None,
                     pipeline=A.FTN_PIPELINE_AUTO, device=-1, film=None, count_traffic=False):
    """Shaped like ao.render_ao: create_scene (unless `scene` is given) + Film (unless `film` is given) + ftn_render_lightpass.  `raw`
    ([H, W, 8] float32) is added into when given, else a zero buffer is.  count_traffic: the shadow rays take the reference-order
    traversal instead of the production any-hit kernels.  Returns (resolved dict, raw sums, stats)."""
    raw, st = F.render_host(PASS, be, builder, cam, res, sampler, tiles=tiles, crop=crop, scene=scene, raw=raw, pipeline=pipeline, device=device, film=film,
                            count_traffic=count_traffic, extra=lambda: index_list(lights))
    return resolve(be, raw), raw, st


def render_lightpass_torch(scene, cam, film, sampler, out, lights=None, tiles=None, pipeline=A.FTN_PIPELINE_AUTO):
    """ftn_render_lightpass_device into `out` (float32 CUDA tensor [H, W, 8], added into) on the current stream of its device."""
    return F.render_torch(PASS, scene, cam, film, sampler, out, tiles=tiles, pipeline=pipeline, extra=lambda: index_list(lights))


def resolve_torch(be, raw, out):
    """ftn_lightpass_resolve_device: raw [..., 8] sums -> out [..., 8] resolved floats, both float32 CUDA tensors, current stream."""
    return F.resolve_torch(PASS, be, raw, out)


# ------------------------------------------------------------------ python -m fountain_amd.lightpass relight
def _parse_light(text):
    """G=FILE:r,g,b -> (G, FILE, (r, g, b)); ValueError otherwise"""
    name, _, rest = text.partition("=")
    path, _, gain = rest.rpartition(":")
    rgb = tuple(float(v) for v in gain.split(","))
    if not name or not path or len(rgb) != 3 or not all(np.isfinite(rgb)):
        raise ValueError(text)
    return name, path, rgb


def relight_files(be, albedo, lights):
    """compose on images: albedo [H, W, 3], lights = list of (lit [H, W, 3], (r, g, b)).  A pixel's coverage counts as 1: where the
    G-buffer recorded no surface its albedo file holds 0, and so does the result."""
    albedo = host_image(albedo, 3)
    h, w = albedo.shape[:2]
    gb12 = np.zeros((h, w, 12), np.float32)
    gb12[..., 0:3], gb12[..., 10] = albedo, 1.0
    res8 = np.zeros((len(lights), h, w, 8), np.float32)
    for g, (lit, _) in enumerate(lights):
        res8[g, ..., 0:3] = host_image(lit, 3, (h, w))
    return compose(be, gb12, res8, [gain for _, gain in lights])


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="fountain_amd.lightpass")
    sub = ap.add_subparsers(dest="command", required=True)
    rl = sub.add_parser("relight", help="sum light-group images, each scaled by a gain, over the albedo: the relighting step on files")
    rl.add_argument("--albedo", required=True, metavar="A.exr", help="the G-buffer's albedo (<name>_albedo.exr of render.py --gbuffer)")
    rl.add_argument("--light", action="append", required=True, metavar="G=FILE:r,g,b", help="a group's <name>_light_<group>.exr and its gain; repeat per group")
    rl.add_argument("-o", "--output", required=True, metavar="out.exr")
    opts = ap.parse_args(argv)
    try:
        lights = [_parse_light(t) for t in opts.light]
    except ValueError as e:
        return refuse("--light takes G=FILE:r,g,b with three finite gains, not %s" % e)
    if not 1 <= len(lights) <= A.FTN_LIGHTPASS_MAX_GROUPS or len({n for n, _, _ in lights}) != len(lights):
        return refuse("relight takes 1 to %d groups of different names" % A.FTN_LIGHTPASS_MAX_GROUPS)
    if not opts.output.endswith(".exr"):
        return refuse("the output must be an .exr file")
    from .api import default_backend, read_exr, write_exr
    be = default_backend()
    albedo = read_exr(opts.albedo, be)
    images = [(read_exr(path, be), gain) for _, path, gain in lights]
    for (name, path, _), (img, _) in zip(lights, images):
        if img.shape != albedo.shape:
            return refuse("%s is %d x %d, the albedo %d x %d" % (path, img.shape[1], img.shape[0], albedo.shape[1], albedo.shape[0]))
    write_exr(opts.output, relight_files(be, albedo, images), be)
    print("relight: %s from %d groups (%s)" % (opts.output, len(lights), ", ".join(n for n, _, _ in lights)), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
