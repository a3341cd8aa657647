"""`python -m fountain_amd.render scene.pbrt [-o out.exr] [--samples N]`: the reference's `render` binary
(src/bin/render.rs:16-104) over the MI355X library -- parse the scene file, PathIntegrator::new(5, 1.0), render, write
Film::into_spectrum_buffer as an OpenEXR file.  `--help` says what each option does; this says what it does not.

Files.  Every extra output stands beside the image, named by beside(): out.exr -> out_albedo.exr, out_normal.exr, out_position.exr,
out_depth.exr (--gbuffer), out_crypto.exr (--idmatte), out_ao.exr and out_bent.exr (--ao), out_light_<group>.exr and
out_lightvis_<group>.exr (--light-groups), out_denoised.exr, out_denoised_guided.exr, out_variance.exr, out_spp.exr (--adaptive),
out_bloom.exr and out.png, with a .png beside each denoised image too, encoded (and bloomed) with the exposure of the main image so
that they compare fairly.  One-channel buffers (depth, AO, visibility, spp) are repeated in R, G and B.  out.exr and every other
OpenEXR file are the same bytes whatever else is asked for.  --compare-to writes no file: it prints the line of
`python -m fountain_amd.metrics`.

What combines with what is the table EXTRAS below and refusal() over it ("The render command line").  The first-hit
passes, the denoisers and --variance work on the image's own camera samples, so they need the default sampler (with --exact-stream a
sample's camera ray depends on everything its tile drew before it) and one GPU.  A wide --pixel-filter mixes the samples of
neighbouring pixels, so every option that assumes that a pixel's samples are its own is refused with it.  --adaptive gives each tile
its own sample count; a G-buffer and the denoisers would have to follow those counts, --variance does (it comes from the same
moments).  --denoise-guided needs 2 samples per pixel, below that a pixel's variance is unknown.  Without --pixel-filter the image is
the reference's: a box of radius 0.5, whatever the file says.

With `--gpus N` (the program starts its N ranks itself, fountain_amd/launch.py) or under `python -m torch.distributed.run
--nproc-per-node N ...` every rank renders the film tiles r, r+N, ... on GPU LOCAL_RANK and the films are merged with the frame's
single reduce (RCCL when every rank has its own GPU, gloo with --dist-backend gloo); rank 0 writes the image.  --threads of the
reference has no meaning here; --gpu picks the HIP device.  --exact-stream renders with the reference's own per-tile RandomSampler
stream (one lane per 16x16 tile: for validation, slow); the default re-seeds per (pixel, sample) so that samples run in parallel (see
DESIGN.md, samplers).
"""
import argparse
import os
import sys
import time
from collections import namedtuple
from types import SimpleNamespace

from . import _abi as A
from . import bloom as B
from . import launch
from ._cli import beside, refuse
from .api import PathIntegrator, PbrtScene, SamplerIntegrator, default_backend, write_exr
from .display import add_arguments as add_display_arguments, display_options_given
from .idmatte import LAYERS


def parser():
    ap = argparse.ArgumentParser(prog="fountain_amd.render")
    ap.add_argument("scene_file")
    ap.add_argument("-o", "--output", dest="image_name", default=None)
    ap.add_argument("--samples", type=int, default=None)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--exact-stream", action="store_true")
    ap.add_argument("--max-depth", type=int, default=5)          # render.rs:79 hard-codes PathIntegrator::new(5, 1.0)
    ap.add_argument("--rr-threshold", type=float, default=1.0)
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"])
    ap.add_argument("--gpus", type=int, default=None, help="render on N GPUs of this node: film tiles r, r+N, ... per rank, one reduce at the end")
    ap.add_argument("--gbuffer", action="store_true", help="also write the first-hit albedo / normal / position / depth buffers as <name>_<buffer>.exr")
    ap.add_argument("--idmatte", default=None, metavar="KIND[,KIND]",
                    help="also write <name>_crypto.exr: Cryptomatte layers of the image's camera samples, one per kind (material, shape, primitive)")
    ap.add_argument("--ao", type=int, nargs="?", const=4, default=None, metavar="RAYS",
                    help="also write <name>_ao.exr and <name>_bent.exr: ambient occlusion and bent normals of the image's camera samples, RAYS (default 4) rays each")
    ap.add_argument("--ao-radius", type=float, default=None, metavar="R", help="with --ao: the length of the occlusion rays (default: unbounded)")
    ap.add_argument("--light-groups", nargs="?", const="kind", default=None, choices=["kind", "each"], metavar="kind|each",
                    help="also write <name>_light_<group>.exr and <name>_lightvis_<group>.exr per group of lights: direct irradiance and visibility of the image's camera samples")
    ap.add_argument("--denoise", action="store_true", help="also write <name>_denoised.exr, the image denoised with the first-hit G-buffer of its camera samples")
    ap.add_argument("--variance", action="store_true", help="also write <name>_variance.exr, the estimated variance of each pixel's mean (r, g, b)")
    ap.add_argument("--denoise-guided", action="store_true",
                    help="also write <name>_denoised_guided.exr, the image denoised with its G-buffer and the variance of each pixel's mean")
    ap.add_argument("--adaptive", type=float, default=None, metavar="T",
                    help="per-tile adaptive sampling up to --samples: stop a tile once its pixels' relative standard error is at most T; also writes <name>_spp.exr")
    ap.add_argument("--min-samples", type=int, default=None, help="with --adaptive: the samples every tile gets first (default 8)")
    ap.add_argument("--pixel-filter", default=None, choices=["scene", "box", "triangle", "gaussian", "mitchell", "sinc"],
                    help="render through this reconstruction filter (scene: the file's PixelFilter statement)")
    ap.add_argument("--filter-width", type=float, nargs="+", default=None, metavar="X", help="with --pixel-filter: the filter's radius, X [Y]")
    ap.add_argument("--png", action="store_true", help="also write <name>.png (and a .png beside each denoised image) through the display stage")
    add_display_arguments(ap)
    B.add_arguments(ap)
    ap.add_argument("--compare-to", default=None, metavar="REF.exr", help="measure the image against this OpenEXR file and print the error measures")
    ap.add_argument("--ssim", action="store_true", help="with --compare-to: SSIM as well")
    return ap


# ------------------------------------------------------------------ the outputs beside the image
def write_outputs(r):
    """Every given row's outputs, in the table's order.  `r` is the finished render: the image `img` as written, what rendered it, and
    what a row leaves for the rows after it -- `shown` and `bloomed` (--bloom), `png` (the PngWriter), `gb` (the G-buffer, rendered once)."""
    for x in EXTRAS:
        if x.write and x.given(r.opts):
            x.write(r)


def write_metrics(r):
    from . import metrics as M
    from .api import read_exr
    m = M.compare(r.be, r.img, read_exr(r.opts.compare_to, r.be), M.MetricsParams(r.be, ssim=r.opts.ssim), device=r.device)
    print("metrics: " + M.report_line(m, r.opts.ssim))


def write_bloom(r):
    """<name>_bloom.exr; the .png files after it are the bloomed images'."""
    p = B.params_from_arguments(r.be, r.opts)
    r.bloomed = lambda a: B.bloom(r.be, a, p, device=r.device)
    r.shown = r.bloomed(r.img)
    write_exr(bloom_path(r.filename), r.shown, r.be)
    print("bloom: %s (strength %.6g, %d levels)" % (bloom_path(r.filename), p.desc.strength, p.desc.levels), file=sys.stderr)


def write_png(r):
    r.png = PngWriter(r.be, r.opts, r.shown)
    r.png.write(r.shown, r.filename)


# The files beside the image, out.exr -> out_denoised.exr and so on; other tools and the tests call these by name.
def gbuffer_paths(filename): return {k: beside(filename, "_%s.exr" % k) for k in ("albedo", "normal", "position", "depth")}
def ao_paths(filename): return {k: beside(filename, "_%s.exr" % k) for k in ("ao", "bent")}
def denoised_path(filename): return beside(filename, "_denoised.exr")
def denoised_guided_path(filename): return beside(filename, "_denoised_guided.exr")
def variance_path(filename): return beside(filename, "_variance.exr")
def bloom_path(filename): return beside(filename, "_bloom.exr")
def spp_path(filename): return beside(filename, "_spp.exr")
def idmatte_path(filename): return beside(filename, "_crypto.exr")
def png_path(exr_name): return beside(exr_name, ".png")


def lightpass_paths(filename, group):
    """out.exr, key -> {"light": out_light_key.exr, "lightvis": out_lightvis_key.exr}.  Not beside(): the name is cut at its last ".exr"
    wherever that stands, so out.exr.tmp gives out_light_key.exr."""
    base = filename[:filename.rindex(".exr")]
    return {k: "%s_%s_%s.exr" % (base, k, group) for k in ("light", "lightvis")}


def gbuffer(r):
    """The first-hit G-buffer of the beauty's camera samples (same film, sampler and tiles), rendered once: (resolved buffers, stats, the
    12 resolved floats per pixel [H, W, 12])."""
    if r.gb is None:
        import numpy as np
        from .gbuffer import CHANNELS, render_gbuffer
        res, _, st = render_gbuffer(r.be, None, r.camera, tuple(r.film.desc.full_resolution), r.sampler, scene=r.scene, film=r.film, device=r.device)
        r.gb = res, st, np.concatenate([res[k] for k in CHANNELS], axis=-1)
    return r.gb


def write_gbuffer(r):
    import numpy as np
    res, st, _ = gbuffer(r)
    paths = gbuffer_paths(r.filename)
    for k in ("albedo", "normal", "position"):
        write_exr(paths[k], res[k], r.be)
    write_exr(paths["depth"], np.repeat(res["depth"], 3, axis=-1), r.be)
    print("G-buffer: %s (%.1f ms on the GPU)" % (", ".join(paths[k] for k in ("albedo", "normal", "position", "depth")), st["kernel_ms"]), file=sys.stderr)


def _write_filtered(r, path, label, filtered):
    """A denoised image as `path`, and with --png its .png beside it at the main image's exposure."""
    t0 = time.time()
    out = filtered()
    write_exr(path, out, r.be)
    print("%s: %s (%.1f ms)" % (label, path, (time.time() - t0) * 1e3), file=sys.stderr)
    if r.png:
        r.png.write(r.bloomed(out), path)


def write_denoised(r):
    """The resolved image denoised with its G-buffer (default parameters)."""
    from .denoise import denoise
    g = gbuffer(r)[2]
    _write_filtered(r, denoised_path(r.filename), "denoised", lambda: denoise(r.be, r.img, g, device=r.device))


def write_denoised_guided(r):
    """The resolved image denoised with its G-buffer and the variance of each pixel's mean (default parameters)."""
    from .denoise import denoise_guided
    g = gbuffer(r)[2]
    _write_filtered(r, denoised_guided_path(r.filename), "denoised (variance-guided)", lambda: denoise_guided(r.be, r.img, g, r.variance, device=r.device))


def write_idmatte(r):
    """The ID mattes of the beauty's camera samples (same film, sampler and tiles), one Cryptomatte layer per kind."""
    from . import idmatte as I
    layers, ms = {}, 0.0
    for kind in idmatte_kinds(r.opts):
        ids, names = I.prim_ids(r.parsed, kind)
        resolved, _, st = I.render_idmatte(r.be, None, r.camera, None, r.sampler, ids, scene=r.scene, film=r.film, device=r.device)
        layers[I.LAYERS[kind]] = (resolved, names)
        ms += st["kernel_ms"]
    path = idmatte_path(r.filename)
    I.write_cryptomatte(path, layers, r.be)
    print("ID mattes: %s (%s; %.1f ms on the GPU)" % (path, ", ".join(layers), ms), file=sys.stderr)


def write_ao(r):
    """The ambient occlusion of the beauty's camera samples: the open fraction in R, G and B (1 where no surface was hit) and the bent normal."""
    import numpy as np
    from .ao import INF, render_ao
    rays, radius = r.opts.ao, r.opts.ao_radius
    res, _, st = render_ao(r.be, None, r.camera, None, r.sampler, rays=rays, radius=INF if radius is None else radius, scene=r.scene, film=r.film, device=r.device)
    paths = ao_paths(r.filename)
    write_exr(paths["ao"], np.repeat(res["ao"], 3, axis=-1), r.be)
    write_exr(paths["bent"], res["bent"], r.be)
    print("ambient occlusion: %s, %s (%d rays per sample, %.1f ms on the GPU, %.1f M occlusion rays/s)" % (
        paths["ao"], paths["bent"], rays, st["kernel_ms"], st["rays_any"] / max(st["any_ms"], 1e-9) / 1e3), file=sys.stderr)


def write_lightpass(r):
    """The light-group AOVs of the film's camera samples, one call per group (lightpass.groups): each group's resolved lit irradiance and
    its visibility (repeated in R, G and B)."""
    import numpy as np
    from .lightpass import groups, render_lightpass
    by_group = groups(r.scene, r.opts.light_groups)
    for name, lights in by_group.items():
        res, _, st = render_lightpass(r.be, None, r.camera, None, r.sampler, lights=lights, scene=r.scene, film=r.film, device=r.device)
        paths = lightpass_paths(r.filename, name)
        write_exr(paths["light"], res["lit"], r.be)
        write_exr(paths["lightvis"], np.repeat(res["visibility"], 3, axis=-1), r.be)
        print("light group %s (%d lights): %s, %s (%.1f ms, %d shadow rays)" % (name, len(lights), paths["light"], paths["lightvis"], st["kernel_ms"], st["rays_any"]),
              file=sys.stderr)
    if not by_group:
        print("light groups: the scene has no lights, nothing written", file=sys.stderr)


def write_spp(r):
    import numpy as np
    write_exr(spp_path(r.filename), np.repeat(r.counts.astype(np.float32)[..., None], 3, axis=-1), r.be)
    print("samples per pixel: %s" % spp_path(r.filename), file=sys.stderr)


def write_variance(r):
    write_exr(variance_path(r.filename), r.variance[..., :3], r.be)
    print("variance: %s" % variance_path(r.filename), file=sys.stderr)


class PngWriter:
    """--png: the display parameters of the command line and the exposure of the main image, which every image written beside it shares."""

    def __init__(self, be, opts, main_img):
        from . import display as D
        self.be, self.device = be, opts.gpu
        self.params = D.params_from_arguments(be, opts)
        hist = D.histogram(be, main_img, device=opts.gpu) if opts.auto_exposure else None
        self.info = D.exposure(be, hist, self.params)
        print("display: scale %.6g%s" % (self.info["scale"], " (automatic, mean log2 luminance %.4f)" % self.info["avg_log2"] if opts.auto_exposure else ""),
              file=sys.stderr)

    def write(self, img, exr_name):
        from . import display as D
        path = png_path(exr_name)
        D.write_png(path, D.encode(self.be, img, self.info["scale"], self.params, device=self.device), self.be, self.params.png_gamma)
        print("png: %s" % path, file=sys.stderr)


# ------------------------------------------------------------------ what is refused
# What is wrong with a row's values once the option is given, or None.
def idmatte_kinds(o): return o.idmatte.split(",")
def _when(wrong, msg): return msg if wrong else None
def _compare_to_wrong(o): return _when(not o.compare_to.endswith(".exr") or not os.path.isfile(o.compare_to), "--compare-to takes an existing .exr file, not %s" % o.compare_to)
def _bloom_wrong(o): return B.refusal(o) or _when(not o.png, "--bloom belongs to --png: it is applied in front of the display stage")
def _png_wrong(o): return _when(o.gamma is not None and o.transfer != "gamma", "--gamma belongs to --transfer gamma")
def _pixel_filter_wrong(o): return _when(o.filter_width is not None and len(o.filter_width) > 2, "--filter-width X [Y] belongs to --pixel-filter")
def _adaptive_wrong(o): return _when(not o.adaptive >= 0.0 or o.adaptive == float("inf"), "--adaptive takes a finite threshold >= 0")
def _ao_wrong(o): return _when(not 1 <= o.ao <= A.FTN_AO_MAX_RAYS or (o.ao_radius is not None and not o.ao_radius > 0.0),
                               "--ao takes 1 to %d rays and --ao-radius a length above zero" % A.FTN_AO_MAX_RAYS)
def _idmatte_wrong(o):
    kinds = idmatte_kinds(o)
    return _when(not all(k in LAYERS for k in kinds) or len(set(kinds)) != len(kinds), "--idmatte takes a list of different kinds out of %s" % ", ".join(LAYERS))


PIXEL_FILTER_SAYS = ("--pixel-filter does not work with %s: a filtered pixel holds samples of its neighbours, and the filtered film renders"
                     " on one GPU with the default sampler")
ADAPTIVE_SAYS = ("--adaptive does not work with %s: it renders each tile at its own sample count on one GPU with the default sampler"
                 " (a G-buffer and the denoiser would have to follow those counts)")

# One row per option that adds outputs or changes how the film is filled, in the order in which their files are written.
#   given(opts)      whether the option is on the command line
#   own_samples      it assumes that a pixel's samples are its own: refused with --pixel-filter
#   one_count        it assumes one sample count for the film: refused with --adaptive
#   sampler          it needs the default sampler: refused with --exact-stream
#   one_gpu          it runs on one GPU: refused under a launcher, and with --gpus -- ANY: whatever N is, MANY: above 1
#   subs(opts)       the names of its sub-options that are given: they belong to it
#   wrong(opts)      what is wrong with its values once it is given, or None
#   says             its own words for what it refuses (default: the words of the need)
#   gpus_says        its own words against --gpus (default: "<flag> <verb> on one GPU: leave out --gpus")
#   verb             what it does on that one GPU
#   write(r)         writes its outputs of a finished render (above)
Extra = namedtuple("Extra", "flag given own_samples one_count sampler one_gpu subs wrong says gpus_says verb write")
ANY, MANY = "any", "many"


def _extra(flag, given, needs="", one_gpu=None, subs=None, wrong=None, says=None, gpus_says=None, verb="renders", write=None):
    gpus_says = gpus_says or (says % "more than one GPU (--gpus)" if says else "%s %s on one GPU: leave out --gpus" % (flag, verb))
    return Extra(flag, given, "own_samples" in needs, "one_count" in needs, "sampler" in needs, one_gpu, subs or (lambda o: []), wrong, says, gpus_says, verb, write)


FIRST_HIT = dict(needs="own_samples one_count sampler", one_gpu=ANY)        # a pass over the image's own camera samples
EXTRAS = (
    _extra("--compare-to", lambda o: o.compare_to is not None, one_gpu=ANY, subs=lambda o: ["--ssim"] * o.ssim, wrong=_compare_to_wrong, verb="measures", write=write_metrics),
    _extra("--bloom", lambda o: o.bloom is not None, subs=B.bloom_options_given, wrong=_bloom_wrong, write=write_bloom),
    _extra("--png", lambda o: o.png, one_gpu=MANY, subs=display_options_given, wrong=_png_wrong, gpus_says="--png encodes on one GPU: leave out --gpus", write=write_png),
    _extra("--pixel-filter", lambda o: o.pixel_filter is not None, needs="sampler", one_gpu=MANY,
           subs=lambda o: ["--filter-width X [Y]"] * (o.filter_width is not None), wrong=_pixel_filter_wrong, says=PIXEL_FILTER_SAYS),
    _extra("--gbuffer", lambda o: o.gbuffer, write=write_gbuffer, **FIRST_HIT),
    _extra("--denoise", lambda o: o.denoise, write=write_denoised, **FIRST_HIT),
    _extra("--denoise-guided", lambda o: o.denoise_guided, write=write_denoised_guided, **FIRST_HIT),
    _extra("--idmatte", lambda o: o.idmatte is not None, wrong=_idmatte_wrong, write=write_idmatte, **FIRST_HIT),
    _extra("--ao", lambda o: o.ao is not None, subs=lambda o: ["--ao-radius"] * (o.ao_radius is not None), wrong=_ao_wrong, write=write_ao, **FIRST_HIT),
    _extra("--light-groups", lambda o: o.light_groups is not None, write=write_lightpass, **FIRST_HIT),
    _extra("--adaptive", lambda o: o.adaptive is not None, needs="own_samples sampler", one_gpu=MANY, subs=lambda o: ["--min-samples"] * (o.min_samples is not None),
           wrong=_adaptive_wrong, says=ADAPTIVE_SAYS, write=write_spp),
    _extra("--variance", lambda o: o.variance, needs="own_samples sampler", one_gpu=ANY, write=write_variance),
)
ROW = {x.flag: x for x in EXTRAS}


def refusal(opts, world=None):
    """Why fountain_amd.render refuses these parsed options, or None: a pure function of them and of the launcher's world size (None:
    started plainly); the only file it looks at is --compare-to's.  In this order: each row's sub-options without it,
    --gpus and its values; what --pixel-filter, then --adaptive, then --exact-stream do not work with; the launcher."""
    on = [x for x in EXTRAS if x.given(opts)]
    for x in EXTRAS:
        subs = x.subs(opts)
        if x not in on and subs:
            return "%s belongs to %s" % (", ".join(subs), x.flag)
        if x in on and x.one_gpu and opts.gpus is not None and (x.one_gpu == ANY or opts.gpus > 1):
            return x.gpus_says
        why = x.wrong(opts) if x in on and x.wrong else None
        if why:
            return why
    for row, need in ((ROW["--pixel-filter"], "own_samples"), (ROW["--adaptive"], "one_count")):
        for x in on if row in on else ():
            if getattr(x, need):
                return row.says % x.flag
    for x in on:
        if x.sampler and opts.exact_stream:
            return x.says % "--exact-stream" if x.says else \
                "%s needs the default sampler: with --exact-stream a sample's camera ray depends on everything its tile drew before it" % x.flag
    # started plainly, main starts --gpus N ranks itself when N is above 1, and is one rank otherwise
    ranks = world if world is not None else max(opts.gpus or 1, 1)
    for x in on:
        if x.one_gpu and world is not None and world > 1:
            return "%s %s on one GPU, not under a launcher of %d ranks" % (x.flag, x.verb, world)
    if opts.gpus is not None and opts.gpus != ranks:
        return "--gpus %d but the launcher started WORLD_SIZE %d ranks" % (opts.gpus, ranks)
    return None


def min_samples(opts, sampler):
    """--min-samples, or 8 (the library's default) but at most the samples per pixel"""
    return opts.min_samples if opts.min_samples is not None else min(8, sampler.desc.samples_per_pixel)


def late_refusal(opts, parsed, be):
    """The refusals that need the parsed scene file, still before a scene is created: (message, None, None), or (None, the sampler, the
    pixel filter or None), which the checks have to build anyway."""
    if opts.compare_to is not None:
        from . import metrics as M
        size, want = M.exr_size(opts.compare_to, be), parsed.film()
        if size != (want.width, want.height) or (opts.ssim and min(size) < A.FTN_METRICS_SSIM_TAPS):
            return "--compare-to %s: %s, the film is %d x %d%s" % (opts.compare_to, "%d x %d pixels" % size if size else "not a readable OpenEXR file",
                                                                   want.width, want.height, " (--ssim needs at least 11 x 11)" if opts.ssim else ""), None, None
    sampler = parsed.sampler(opts.samples, indexed=not opts.exact_stream)
    spp = sampler.desc.samples_per_pixel
    if opts.denoise_guided and spp < 2:
        return "--denoise-guided needs at least 2 samples per pixel: a pixel's variance is unknown below that (here %d)" % spp, None, None
    if opts.adaptive is not None and not 2 <= min_samples(opts, sampler) <= spp:
        return "--adaptive needs 2 <= --min-samples <= samples per pixel (here %d and %d)" % (min_samples(opts, sampler), spp), None, None
    filt = pixel_filter(opts, parsed, be)
    if opts.pixel_filter == "scene" and filt is None:
        return "--pixel-filter scene, but %s has no PixelFilter statement" % opts.scene_file, None, None
    return None, sampler, filt


def pixel_filter(opts, parsed, be):
    """--pixel-filter's Filter with --filter-width's radius; None without the option, or where `scene` finds no statement in the file"""
    if opts.pixel_filter is None:
        return None
    from .filters import Filter
    width = None if opts.filter_width is None else (opts.filter_width[0], opts.filter_width[-1])
    if opts.pixel_filter != "scene":
        return Filter(opts.pixel_filter, width, be=be)
    filt = Filter.from_pbrt(parsed)
    if filt is not None and width is not None:
        filt.desc.radius[0], filt.desc.radius[1] = width
    return filt


# ------------------------------------------------------------------ the render


Rendered = namedtuple("Rendered", "film stats variance counts")      # variance: with moments; counts: with --adaptive; else None


def render_image(be, opts, integrator, scene, film, sampler, filt, world, rank):
    """Fills the film one of five ways: over the ranks of a launcher, through a pixel filter, adaptively, with moments, or plainly.
    Returns a Rendered, or None on a rank that has nothing to write."""
    camera, common = integrator.camera, dict(scene=scene, film=film, device=opts.gpu)
    variance = counts = None
    if world > 1:
        st = render_ranks(opts, integrator, scene, film, sampler, world, rank)
        if rank != 0:
            return None
    elif filt is not None:
        from .filters import filtered_film, render_filtered
        film = filtered_film(be, filt, film=film)
        _, _, st = render_filtered(be, None, camera, None, integrator.radiance, sampler, filt, scene=scene, film=film, device=opts.gpu)
    elif opts.adaptive is not None:
        # each tile at its own sample count, with the moments that decided it beside the beauty
        from .adaptive import params, render_adaptive
        from .moments import resolve
        p = params(be, threshold=opts.adaptive, min_samples=min_samples(opts, sampler))
        _, moments, counts, ainfo, st = render_adaptive(be, None, camera, None, integrator.radiance, sampler, p, **common)
        if opts.variance:
            variance = resolve(be, film.pixels, moments)
        print("adaptive: %d rounds, %d of %d tiles at %d samples, %.2f samples per pixel" % (
            ainfo["rounds"], ainfo["tiles_at_max"], ainfo["tiles"], sampler.desc.samples_per_pixel,
            ainfo["pixel_samples"] / max(1, counts.size)), file=sys.stderr)
    elif opts.variance or opts.denoise_guided:
        # the beauty of ftn_render, bit for bit, with the moments of its samples beside it
        from .moments import render_moments
        variance, _, _, st = render_moments(be, None, camera, None, integrator.radiance, sampler, **common)
    else:
        st = integrator.render_parallel(scene, film, sampler, device=opts.gpu)
    return Rendered(film, st, variance, counts)


def render_ranks(opts, integrator, scene, film, sampler, world, rank):
    """This rank's tiles, then the films of all ranks merged into `film` with the frame's single reduce."""
    import torch
    import torch.distributed as dist
    from .distributed import merge_film, tile_shard
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if opts.dist_backend == "nccl":
        torch.cuda.set_device(opts.gpu)
        dist.init_process_group("nccl", device_id=torch.device("cuda", opts.gpu))
    else:
        dist.init_process_group("gloo")
    st = integrator.render_parallel(scene, film, sampler, tiles=tile_shard(rank, world), device=opts.gpu)
    t = torch.from_numpy(film.pixels)
    if opts.dist_backend == "nccl":
        t = t.cuda(opts.gpu)
    merge_film(t)
    film.pixels[...] = t.cpu().numpy()
    dist.barrier()
    dist.destroy_process_group()
    return st


def main(argv=None):
    opts = parser().parse_args(argv)
    env_world = launch.world_from_env()
    why = refusal(opts, env_world and env_world[0])
    if why:
        return refuse(why)
    if env_world is None and opts.gpus is not None and opts.gpus > 1:
        # started plainly: start the N ranks as a child process (before anything here has touched HIP) and hand back its exit code
        return launch.spawn_ranks(opts.gpus, sys.argv[1:] if argv is None else list(argv), module="fountain_amd.render")
    world, rank = (env_world[0], env_world[1]) if env_world is not None else (1, 0)
    if world > 1:
        opts.gpu = int(os.environ.get("LOCAL_RANK", "0")) if opts.dist_backend == "nccl" else opts.gpu

    be = default_backend()
    parsed = PbrtScene(opts.scene_file, be)
    filename = opts.image_name or parsed.film_name
    if ".exr" not in filename:
        raise SystemExit("output must be an .exr file (render.rs:53)")
    why, sampler, filt = late_refusal(opts, parsed, be)
    if why:
        return refuse(why)
    scene = parsed.create_scene(device=opts.gpu)
    film = parsed.film()
    integrator = SamplerIntegrator(parsed.camera, PathIntegrator.new(opts.max_depth, opts.rr_threshold))
    info = scene.info()
    print("scene: %d primitives, %d BVH nodes, %d lights" % (info["n_prims"], info["n_nodes"], info["n_lights"]), file=sys.stderr)
    t0 = time.time()
    done = render_image(be, opts, integrator, scene, film, sampler, filt, world, rank)
    if done is None:
        return 0
    dt = time.time() - t0
    rays = done.stats["rays_closest"] + done.stats["rays_any"]
    print("Completed rendering in %.3f s (%.1f Mrays/s%s)" % (dt, rays / dt / 1e6, " on rank 0 of %d" % world if world > 1 else ""), file=sys.stderr)
    img, _ = done.film.into_spectrum_buffer()
    write_exr(filename, img, be)
    write_outputs(SimpleNamespace(be=be, opts=opts, device=opts.gpu, parsed=parsed, camera=parsed.camera, scene=scene, sampler=sampler, filename=filename, img=img,
                                  film=done.film, variance=done.variance, counts=done.counts, shown=img, bloomed=lambda a: a, png=None, gb=None))
    return 0


if __name__ == "__main__":
    sys.exit(main())
