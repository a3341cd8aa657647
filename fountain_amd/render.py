"""`python -m fountain_amd.render scene.pbrt [-o out.exr] [--samples N]`: the reference's `render` binary
(src/bin/render.rs:16-104) over the MI355X library -- parse the scene file, PathIntegrator::new(5, 1.0), render, write
Film::into_spectrum_buffer as an OpenEXR file.

--threads of the reference has no meaning here; --gpu picks the HIP device.  With `--gpus N` (the program starts its N ranks itself,
fountain_amd/launch.py) or started under `python -m torch.distributed.run --nproc-per-node N …` every rank renders the film tiles r, r+N, … on GPU LOCAL_RANK and the films are merged with the frame's single
reduce (RCCL when every rank has its own GPU, gloo with --dist-backend gloo); rank 0 writes the image.  --exact-stream renders with the reference's own
per-tile RandomSampler stream (one lane per 16x16 tile: for validation, slow); the default re-seeds per (pixel, sample) so that
samples run in parallel (samplers).  --gbuffer also writes the first-hit G-buffer of the same camera samples
(fountain_amd/gbuffer.py) beside the image: <name>_albedo.exr, <name>_normal.exr, <name>_position.exr and <name>_depth.exr (camera-space
depth repeated in R, G and B); it needs the default sampler and one GPU.  --idmatte KIND[,KIND] (material, shape, primitive) also
writes <name>_crypto.exr: the ID mattes of the same camera samples (fountain_amd/idmatte.py) as Cryptomatte layers CryptoMaterial,
CryptoObject and CryptoPrimitive, one per kind; it has the same needs as --gbuffer.  --ao [RAYS] (default 4, at most 64) also writes the
ambient occlusion of the same camera samples (fountain_amd/ao.py), RAYS cosine-distributed occlusion rays per sample of at most
--ao-radius R (default: unbounded): <name>_ao.exr (the open fraction in R, G and B, 1 where no surface was hit) and <name>_bent.exr (the
bent normal); it has the same needs as --gbuffer.  --light-groups [kind|each] (default kind) also writes the light-group AOVs of the same
camera samples (fountain_amd/lightpass.py), one light sample and one shadow ray per sample and group: <name>_light_<group>.exr (the
direct irradiance the group's lights leave on the first surface, shadows included) and <name>_lightvis_<group>.exr (the fraction of that
light the scene lets through, in R, G and B); `kind` makes one group per kind of light the scene has (point, distant, infinite, area),
`each` one per explicit light (light<i>) and one for the area lights.  `python -m fountain_amd.lightpass relight` sums such files over the
albedo with a gain per group.  It has the same needs as --gbuffer.  --denoise then renders that G-buffer (also without
--gbuffer) and writes <name>_denoised.exr: the image filtered by the edge-avoiding a-trous denoiser (fountain_amd/denoise.py, default
parameters); the image itself is written unchanged.  It has the same needs as --gbuffer.  --variance renders the image together with
the second moments of its camera samples (fountain_amd/moments.py), the same pixels bit for bit, and writes <name>_variance.exr: the
estimated variance of each pixel's mean in R, G and B (+inf where a pixel has fewer than 2 samples).  It has the same needs as --gbuffer.
--denoise-guided renders the image with those moments (as --variance does) and the G-buffer, and writes <name>_denoised_guided.exr:
the image filtered by the variance-guided a-trous denoiser (fountain_amd/denoise.py, default parameters); the image itself is written
unchanged.  It has the needs of --gbuffer and at least 2 samples per pixel, and combines with --variance and --denoise.
--adaptive T renders with per-tile adaptive sampling (fountain_amd/adaptive.py): every 16x16 tile gets --min-samples samples (default
8, at most the samples per pixel), then twice as many, and so on up to --samples, until the estimated relative standard error of
each of its pixels' mean luminance is at most T.  It writes <name>_spp.exr beside the image: each pixel's final sample count in R, G and B.  --variance works with it (from
the same moments); --gbuffer, --idmatte, --denoise, --exact-stream and more than one GPU do not.
--pixel-filter {scene,box,triangle,gaussian,mitchell,sinc} renders the image through a reconstruction filter (fountain_amd/filters.py):
`scene` takes the file's PixelFilter statement (an error if it has none), the others the defaults of that filter; --filter-width X [Y]
sets the radius.  A wide filter mixes the samples of neighbouring pixels, so --gbuffer, --idmatte, --denoise, --denoise-guided, --variance and
--adaptive, which assume that a pixel's samples are its own, are refused with it, as are --exact-stream and more than one GPU.
Without the option the image is the reference's: a box of radius 0.5, whatever the file says.
--png also writes <name>.png beside <name>.exr through the display stage (fountain_amd/display.py): --exposure EV (default 0) or
--auto-exposure (from the image's luminance histogram), --tonemap {linear,reinhard,aces,hable} (default aces), --transfer
{srgb,gamma,linear} (default srgb) with --gamma G, and --dither.  <name>_denoised.exr and <name>_denoised_guided.exr get a .png beside
them too, encoded with the exposure of the main image so that they compare fairly; the G-buffer, variance and spp files get none.  The
display options need --png, and --png renders on one GPU.  The OpenEXR files are the same bytes with and without it.
--bloom [STRENGTH] (default 0.04) blooms the linear image in front of the display stage (fountain_amd/bloom.py) with --bloom-levels N,
--bloom-scatter S, --bloom-threshold T, --bloom-knee K and --bloom-karis, and writes it as <name>_bloom.exr; <name>.png is then the
bloomed image's, its histogram and so the automatic exposure included, and the denoised images' .png files are bloomed too before they
are encoded at that exposure.  <name>.exr and every other file stay the same bytes.  --bloom needs --png and one GPU, and its
sub-options need --bloom.
--compare-to REF.exr [--ssim] measures the image just written against REF.exr (fountain_amd/metrics.py) and prints the line of
`python -m fountain_amd.metrics`: RMSE, MSE, MAE, relMSE, SMAPE, PSNR, the largest difference, with --ssim SSIM, and how many pixels
differ.  REF.exr must exist and have the film's size, and the option renders on one GPU; all of that is checked before anything is
rendered.  It writes no file, and without it nothing changes.
"""
import argparse
import sys
import time

from . import _abi as A
from .api import PathIntegrator, PbrtScene, SamplerIntegrator, default_backend, write_exr


def main(argv=None):
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
    from .display import add_arguments as add_display_arguments, display_options_given
    add_display_arguments(ap)
    from . import bloom as B
    B.add_arguments(ap)
    ap.add_argument("--compare-to", default=None, metavar="REF.exr", help="measure the image against this OpenEXR file and print the error measures")
    ap.add_argument("--ssim", action="store_true", help="with --compare-to: SSIM as well")
    opts = ap.parse_args(argv)
    if opts.ssim and opts.compare_to is None:
        print("error: --ssim belongs to --compare-to", file=sys.stderr)
        return 2
    if opts.compare_to is not None:
        import os.path
        if opts.gpus is not None:
            print("error: --compare-to measures on one GPU: leave out --gpus", file=sys.stderr)
            return 2
        if not opts.compare_to.endswith(".exr") or not os.path.isfile(opts.compare_to):
            print("error: --compare-to takes an existing .exr file, not %s" % opts.compare_to, file=sys.stderr)
            return 2
    if B.refusal(opts):
        print("error: %s" % B.refusal(opts), file=sys.stderr)
        return 2
    if opts.bloom is not None and not opts.png:
        print("error: --bloom belongs to --png: it is applied in front of the display stage", file=sys.stderr)
        return 2
    if not opts.png and display_options_given(opts):
        print("error: %s belongs to --png" % ", ".join(display_options_given(opts)), file=sys.stderr)
        return 2
    if opts.gamma is not None and opts.transfer != "gamma":
        print("error: --gamma belongs to --transfer gamma", file=sys.stderr)
        return 2
    if opts.png and opts.gpus is not None and opts.gpus > 1:
        print("error: --png encodes on one GPU: leave out --gpus", file=sys.stderr)
        return 2
    if opts.filter_width is not None and (opts.pixel_filter is None or len(opts.filter_width) > 2):
        print("error: --filter-width X [Y] belongs to --pixel-filter", file=sys.stderr)
        return 2
    if opts.ao_radius is not None and opts.ao is None:
        print("error: --ao-radius belongs to --ao", file=sys.stderr)
        return 2
    if opts.ao is not None and (not 1 <= opts.ao <= A.FTN_AO_MAX_RAYS or (opts.ao_radius is not None and not opts.ao_radius > 0.0)):
        print("error: --ao takes 1 to %d rays and --ao-radius a length above zero" % A.FTN_AO_MAX_RAYS, file=sys.stderr)
        return 2
    if opts.idmatte is not None:
        from .idmatte import LAYERS
        opts.idmatte = opts.idmatte.split(",")
        if not all(k in LAYERS for k in opts.idmatte) or len(set(opts.idmatte)) != len(opts.idmatte):
            print("error: --idmatte takes a list of different kinds out of %s" % ", ".join(LAYERS), file=sys.stderr)
            return 2
    if opts.pixel_filter is not None:
        for flag, on in (("--gbuffer", opts.gbuffer), ("--idmatte", opts.idmatte is not None), ("--ao", opts.ao is not None), ("--light-groups", opts.light_groups is not None), ("--denoise", opts.denoise), ("--denoise-guided", opts.denoise_guided), ("--variance", opts.variance),
                         ("--adaptive", opts.adaptive is not None), ("--exact-stream", opts.exact_stream),
                         ("more than one GPU (--gpus)", opts.gpus is not None and opts.gpus > 1)):
            if on:
                print("error: --pixel-filter does not work with %s: a filtered pixel holds samples of its neighbours, and the filtered film renders"
                      " on one GPU with the default sampler" % flag, file=sys.stderr)
                return 2
    if opts.min_samples is not None and opts.adaptive is None:
        print("error: --min-samples belongs to --adaptive", file=sys.stderr)
        return 2
    if opts.adaptive is not None:
        for flag, on in (("--exact-stream", opts.exact_stream), ("--gbuffer", opts.gbuffer), ("--idmatte", opts.idmatte is not None), ("--ao", opts.ao is not None), ("--light-groups", opts.light_groups is not None), ("--denoise", opts.denoise),
                         ("--denoise-guided", opts.denoise_guided), ("more than one GPU (--gpus)", opts.gpus is not None and opts.gpus > 1)):
            if on:
                print("error: --adaptive does not work with %s: it renders each tile at its own sample count on one GPU with the default sampler"
                      " (a G-buffer and the denoiser would have to follow those counts)" % flag, file=sys.stderr)
                return 2
        if not opts.adaptive >= 0.0 or opts.adaptive == float("inf"):
            print("error: --adaptive takes a finite threshold >= 0", file=sys.stderr)
            return 2
    for flag, on in (("--gbuffer", opts.gbuffer), ("--idmatte", opts.idmatte is not None), ("--ao", opts.ao is not None), ("--light-groups", opts.light_groups is not None), ("--denoise", opts.denoise), ("--variance", opts.variance),
                     ("--denoise-guided", opts.denoise_guided)):
        if on and opts.exact_stream:
            print("error: %s needs the default sampler: with --exact-stream a sample's camera ray depends on everything its tile drew before it" % flag, file=sys.stderr)
            return 2
        if on and opts.gpus is not None:
            print("error: %s renders on one GPU: leave out --gpus" % flag, file=sys.stderr)
            return 2
    import os
    from .launch import spawn_ranks, world_from_env
    env_world = world_from_env()
    if env_world is None and opts.gpus is not None and opts.gpus > 1:
        # started plainly: start the N ranks as a child process (before anything here has touched HIP) and hand back its exit code
        return spawn_ranks(opts.gpus, sys.argv[1:] if argv is None else list(argv), module="fountain_amd.render")
    world, rank = (env_world[0], env_world[1]) if env_world is not None else (1, 0)
    if (opts.gbuffer or opts.idmatte is not None or opts.ao is not None or opts.light_groups is not None or opts.denoise or opts.variance or opts.denoise_guided or opts.adaptive is not None or opts.pixel_filter is not None
            or opts.png) and world > 1:
        flag = "--png" if opts.png else "--gbuffer" if opts.gbuffer else "--idmatte" if opts.idmatte is not None else "--ao" if opts.ao is not None else "--light-groups" if opts.light_groups is not None else "--denoise" if opts.denoise else "--variance" if opts.variance else \
            "--denoise-guided" if opts.denoise_guided else "--adaptive" if opts.adaptive is not None else "--pixel-filter"
        print("error: %s renders on one GPU, not under a launcher of %d ranks" % (flag, world), file=sys.stderr)
        return 2
    if opts.compare_to is not None and world > 1:
        print("error: --compare-to measures on one GPU, not under a launcher of %d ranks" % world, file=sys.stderr)
        return 2
    if opts.gpus is not None and opts.gpus != world:
        print("error: --gpus %d but the launcher started WORLD_SIZE %d ranks" % (opts.gpus, world), file=sys.stderr)
        return 2
    if world > 1:
        opts.gpu = int(os.environ.get("LOCAL_RANK", "0")) if opts.dist_backend == "nccl" else opts.gpu

    be = default_backend()
    parsed = PbrtScene(opts.scene_file, be)
    filename = opts.image_name or parsed.film_name
    if ".exr" not in filename:
        raise SystemExit("output must be an .exr file (render.rs:53)")
    if opts.compare_to is not None:
        from . import metrics as M
        size, want = M.exr_size(opts.compare_to, be), parsed.film()
        if size != (want.width, want.height) or (opts.ssim and min(size) < A.FTN_METRICS_SSIM_TAPS):
            print("error: --compare-to %s: %s, the film is %d x %d%s" % (opts.compare_to, "%d x %d pixels" % size if size else "not a readable OpenEXR file",
                                                                         want.width, want.height, " (--ssim needs at least 11 x 11)" if opts.ssim else ""), file=sys.stderr)
            return 2
    sampler = parsed.sampler(opts.samples, indexed=not opts.exact_stream)
    if opts.denoise_guided and sampler.desc.samples_per_pixel < 2:
        print("error: --denoise-guided needs at least 2 samples per pixel: a pixel's variance is unknown below that (here %d)"
              % sampler.desc.samples_per_pixel, file=sys.stderr)
        return 2
    if opts.adaptive is not None:
        # min_samples: --min-samples, or 8 (the library's default) but at most the samples per pixel
        n_max = sampler.desc.samples_per_pixel
        opts.min_samples = opts.min_samples if opts.min_samples is not None else min(8, n_max)
        if not 2 <= opts.min_samples <= n_max:
            print("error: --adaptive needs 2 <= --min-samples <= samples per pixel (here %d and %d)" % (opts.min_samples, n_max), file=sys.stderr)
            return 2
    filt = None
    if opts.pixel_filter is not None:
        from .filters import Filter
        if opts.pixel_filter == "scene":
            filt = Filter.from_pbrt(parsed)
            if filt is None:
                print("error: --pixel-filter scene, but %s has no PixelFilter statement" % opts.scene_file, file=sys.stderr)
                return 2
            if opts.filter_width is not None:
                filt.desc.radius[0], filt.desc.radius[1] = opts.filter_width[0], opts.filter_width[-1]
        else:
            filt = Filter(opts.pixel_filter, None if opts.filter_width is None else (opts.filter_width[0], opts.filter_width[-1]), be=be)
    scene = parsed.create_scene(device=opts.gpu)
    film = parsed.film()
    integrator = SamplerIntegrator(parsed.camera, PathIntegrator.new(opts.max_depth, opts.rr_threshold))
    info = scene.info()
    print("scene: %d primitives, %d BVH nodes, %d lights" % (info["n_prims"], info["n_nodes"], info["n_lights"]), file=sys.stderr)
    t0 = time.time()
    if world > 1:
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
        if rank != 0:
            return 0
    elif filt is not None:
        from .filters import filtered_film, render_filtered
        film = filtered_film(be, filt, film=film)
        _, _, st = render_filtered(be, None, parsed.camera, None, integrator.radiance, sampler, filt, scene=scene, film=film, device=opts.gpu)
    elif opts.adaptive is not None:
        # each tile at its own sample count, with the moments that decided it beside the beauty
        from .adaptive import params, render_adaptive
        from .moments import resolve
        kw = dict(threshold=opts.adaptive, min_samples=opts.min_samples)
        _, moments, counts, ainfo, st = render_adaptive(be, None, parsed.camera, None, integrator.radiance, sampler, params(be, **kw), scene=scene,
                                                        film=film, device=opts.gpu)
        if opts.variance:
            variance = resolve(be, film.pixels, moments)
        print("adaptive: %d rounds, %d of %d tiles at %d samples, %.2f samples per pixel" % (
            ainfo["rounds"], ainfo["tiles_at_max"], ainfo["tiles"], sampler.desc.samples_per_pixel,
            ainfo["pixel_samples"] / max(1, counts.size)), file=sys.stderr)
    elif opts.variance or opts.denoise_guided:
        # the beauty of ftn_render, bit for bit, with the moments of its samples beside it
        from .moments import render_moments
        variance, _, _, st = render_moments(be, None, parsed.camera, None, integrator.radiance, sampler, scene=scene, film=film, device=opts.gpu)
    else:
        st = integrator.render_parallel(scene, film, sampler, device=opts.gpu)
    dt = time.time() - t0
    rays = st["rays_closest"] + st["rays_any"]
    print("Completed rendering in %.3f s (%.1f Mrays/s%s)" % (dt, rays / dt / 1e6, " on rank 0 of %d" % world if world > 1 else ""), file=sys.stderr)
    img, (w, h) = film.into_spectrum_buffer()
    write_exr(filename, img, be)
    if opts.compare_to is not None:
        from .api import read_exr
        r = M.compare(be, img, read_exr(opts.compare_to, be), M.MetricsParams(be, ssim=opts.ssim), device=opts.gpu)
        print("metrics: " + M.report_line(r, opts.ssim))
    bloom_params = B.params_from_arguments(be, opts) if opts.bloom is not None else None
    bloomed = (lambda a: B.bloom(be, a, bloom_params, device=opts.gpu)) if bloom_params else (lambda a: a)
    shown = bloomed(img)
    if bloom_params:
        write_exr(bloom_path(filename), shown, be)
        print("bloom: %s (strength %.6g, %d levels)" % (bloom_path(filename), bloom_params.desc.strength, bloom_params.desc.levels), file=sys.stderr)
    png = PngWriter(be, opts, shown) if opts.png else None
    if png:
        png.write(shown, filename)
    if opts.gbuffer or opts.denoise or opts.denoise_guided:
        gb = write_gbuffer(be, scene, parsed.camera, film, sampler, filename, opts.gpu, write=opts.gbuffer)
        if opts.denoise:
            out = write_denoised(be, img, gb, filename, opts.gpu)
            if png:
                png.write(bloomed(out), denoised_path(filename))
        if opts.denoise_guided:
            out = write_denoised_guided(be, img, gb, variance, filename, opts.gpu)
            if png:
                png.write(bloomed(out), denoised_guided_path(filename))
    if opts.idmatte is not None:
        write_idmatte(be, scene, parsed, film, sampler, filename, opts.gpu, opts.idmatte)
    if opts.ao is not None:
        write_ao(be, scene, parsed.camera, film, sampler, filename, opts.gpu, opts.ao, opts.ao_radius)
    if opts.light_groups is not None:
        write_lightpass(be, scene, parsed.camera, film, sampler, filename, opts.gpu, opts.light_groups)
    if opts.adaptive is not None:
        import numpy as np
        path = spp_path(filename)
        write_exr(path, np.repeat(counts.astype(np.float32)[..., None], 3, axis=-1), be)
        print("samples per pixel: %s" % path, file=sys.stderr)
    if opts.variance:
        path = variance_path(filename)
        write_exr(path, variance[..., :3], be)
        print("variance: %s" % path, file=sys.stderr)
    return 0


def gbuffer_paths(filename):
    """out.exr -> {"albedo": out_albedo.exr, ...}"""
    base = filename[:-4] if filename.endswith(".exr") else filename
    return {k: "%s_%s.exr" % (base, k) for k in ("albedo", "normal", "position", "depth")}


def denoised_path(filename):
    """out.exr -> out_denoised.exr"""
    base = filename[:-4] if filename.endswith(".exr") else filename
    return "%s_denoised.exr" % base


def denoised_guided_path(filename):
    """out.exr -> out_denoised_guided.exr"""
    base = filename[:-4] if filename.endswith(".exr") else filename
    return "%s_denoised_guided.exr" % base


def variance_path(filename):
    """out.exr -> out_variance.exr"""
    base = filename[:-4] if filename.endswith(".exr") else filename
    return "%s_variance.exr" % base


def bloom_path(filename):
    """out.exr -> out_bloom.exr"""
    base = filename[:-4] if filename.endswith(".exr") else filename
    return "%s_bloom.exr" % base


def spp_path(filename):
    """out.exr -> out_spp.exr"""
    base = filename[:-4] if filename.endswith(".exr") else filename
    return "%s_spp.exr" % base


def write_gbuffer(be, scene, camera, film, sampler, filename, device, write=True):
    """The first-hit G-buffer of the beauty's camera samples (same film, sampler and tiles), resolved and (with `write`) written beside
    the image.  Returns the 12 resolved floats per pixel, [H, W, 12]."""
    import numpy as np
    from .gbuffer import CHANNELS, render_gbuffer
    res, _, st = render_gbuffer(be, None, camera, tuple(film.desc.full_resolution), sampler, scene=scene, film=film, device=device)
    if write:
        paths = gbuffer_paths(filename)
        for k in ("albedo", "normal", "position"):
            write_exr(paths[k], res[k], be)
        write_exr(paths["depth"], np.repeat(res["depth"], 3, axis=-1), be)
        print("G-buffer: %s (%.1f ms on the GPU)" % (", ".join(paths[k] for k in ("albedo", "normal", "position", "depth")), st["kernel_ms"]), file=sys.stderr)
    return np.concatenate([res[k] for k in CHANNELS], axis=-1)


def idmatte_path(filename):
    """out.exr -> out_crypto.exr"""
    base = filename[:-4] if filename.endswith(".exr") else filename
    return "%s_crypto.exr" % base


def write_idmatte(be, scene, parsed, film, sampler, filename, device, kinds):
    """The ID mattes of the beauty's camera samples (same film, sampler and tiles), one Cryptomatte layer per kind, written as
    <name>_crypto.exr."""
    from . import idmatte as I
    layers, ms = {}, 0.0
    for kind in kinds:
        ids, names = I.prim_ids(parsed, kind)
        resolved, _, st = I.render_idmatte(be, None, parsed.camera, None, sampler, ids, scene=scene, film=film, device=device)
        layers[I.LAYERS[kind]] = (resolved, names)
        ms += st["kernel_ms"]
    path = idmatte_path(filename)
    I.write_cryptomatte(path, layers, be)
    print("ID mattes: %s (%s; %.1f ms on the GPU)" % (path, ", ".join(layers), ms), file=sys.stderr)


def lightpass_paths(filename, group):
    """out.exr, key -> {"light": out_light_key.exr, "lightvis": out_lightvis_key.exr}"""
    base = filename[:filename.rindex(".exr")]
    return {k: "%s_%s_%s.exr" % (base, k, group) for k in ("light", "lightvis")}


def write_lightpass(be, scene, camera, film, sampler, filename, device, by):
    """Renders the light-group AOVs of the film's camera samples, one call per group (lightpass.groups), and writes each group's resolved
    lit irradiance and its visibility (repeated in R, G and B).  Returns {group: resolved dict}."""
    import numpy as np
    from .lightpass import groups, render_lightpass
    out = {}
    for name, lights in groups(scene, by).items():
        res, _, st = render_lightpass(be, None, camera, None, sampler, lights=lights, scene=scene, film=film, device=device)
        paths = lightpass_paths(filename, name)
        write_exr(paths["light"], res["lit"], be)
        write_exr(paths["lightvis"], np.repeat(res["visibility"], 3, axis=-1), be)
        print("light group %s (%d lights): %s, %s (%.1f ms, %d shadow rays)" % (name, len(lights), paths["light"], paths["lightvis"], st["kernel_ms"], st["rays_any"]),
              file=sys.stderr)
        out[name] = res
    if not out:
        print("light groups: the scene has no lights, nothing written", file=sys.stderr)
    return out


def ao_paths(filename):
    """out.exr -> {"ao": out_ao.exr, "bent": out_bent.exr}"""
    base = filename[:-4] if filename.endswith(".exr") else filename
    return {k: "%s_%s.exr" % (base, k) for k in ("ao", "bent")}


def write_ao(be, scene, camera, film, sampler, filename, device, rays, radius=None):
    """The ambient occlusion of the beauty's camera samples (same film, sampler and tiles), written beside the image: the open fraction
    in R, G and B (1 where no surface was hit) and the bent normal."""
    import numpy as np
    from .ao import INF, render_ao
    res, _, st = render_ao(be, None, camera, None, sampler, rays=rays, radius=INF if radius is None else radius, scene=scene, film=film, device=device)
    paths = ao_paths(filename)
    write_exr(paths["ao"], np.repeat(res["ao"], 3, axis=-1), be)
    write_exr(paths["bent"], res["bent"], be)
    print("ambient occlusion: %s, %s (%d rays per sample, %.1f ms on the GPU, %.1f M occlusion rays/s)" % (
        paths["ao"], paths["bent"], rays, st["kernel_ms"], st["rays_any"] / max(st["any_ms"], 1e-9) / 1e3), file=sys.stderr)
    return res


def write_denoised(be, img, gb12, filename, device):
    """The resolved image denoised with its G-buffer (default parameters), written as <name>_denoised.exr."""
    from .denoise import denoise
    t0 = time.time()
    out = denoise(be, img, gb12, device=device)
    path = denoised_path(filename)
    write_exr(path, out, be)
    print("denoised: %s (%.1f ms)" % (path, (time.time() - t0) * 1e3), file=sys.stderr)
    return out


def write_denoised_guided(be, img, gb12, var4, filename, device):
    """The resolved image denoised with its G-buffer and the variance of each pixel's mean (default parameters), written as
    <name>_denoised_guided.exr."""
    from .denoise import denoise_guided
    t0 = time.time()
    out = denoise_guided(be, img, gb12, var4, device=device)
    path = denoised_guided_path(filename)
    write_exr(path, out, be)
    print("denoised (variance-guided): %s (%.1f ms)" % (path, (time.time() - t0) * 1e3), file=sys.stderr)
    return out


def png_path(exr_name):
    """out.exr -> out.png"""
    return (exr_name[:-4] if exr_name.endswith(".exr") else exr_name) + ".png"


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


if __name__ == "__main__":
    sys.exit(main())
