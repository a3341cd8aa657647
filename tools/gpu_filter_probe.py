"""Cost of the reconstruction-filtered film (ftn_render_filtered_device) on the config-5 scene next to the beauty step alone
(ftn_render_device), 16 spp, PathIntegrator(5, 1.0), all into device buffers:
  python tools/gpu_filter_probe.py [--res 4096] [--reps 3] [--out profiles/filter/probe.json]
kernel_ms is the whole call (HIP events on its stream); an overhead is the difference of the medians.  The filtered calls render the
film of their own radius (more sample-bounds pixels than the box's), so each is also compared with ftn_render_device over that film."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=4096)
    ap.add_argument("--copies", type=int, default=2309)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter", "probe.json"))
    a = ap.parse_args()
    import torch
    from fountain_amd import Film, PathIntegrator, RandomSampler, SamplerIntegrator, default_backend, scenes
    from fountain_amd import filters as FL
    be = default_backend()
    t0 = time.time()
    b, cam, res = scenes.instanced_cubes(be, n_copies=a.copies, res=(a.res, a.res))
    scene = b.create_scene()
    out = {"scene": "config 5: %d copies of rounded_cube, %dx%d film, %d spp" % (a.copies, a.res, a.res, a.spp), "scene_build_s": round(time.time() - t0, 1), "reps": a.reps}
    integ = PathIntegrator(5, 1.0)
    smp = RandomSampler(a.spp, 0, indexed=True)
    film = Film(be, res)
    px = torch.zeros((film.height, film.width, 4), dtype=torch.float32, device="cuda:0")
    si = SamplerIntegrator(cam, integ)
    stream = torch.cuda.current_stream().cuda_stream
    gauss, sinc = FL.Filter("gaussian", be=be), FL.Filter("sinc", be=be)
    films = {"gaussian_r2": FL.filtered_film(be, gauss, res), "sinc_r4": FL.filtered_film(be, sinc, res)}
    runs_of = [("beauty", lambda: si.render_device(scene, film, smp, px.data_ptr(), stream)),
               ("filtered_gaussian_r2", lambda: FL.render_filtered_torch(scene, cam, films["gaussian_r2"], integ, smp, gauss, px)),
               ("beauty_box_r2", lambda: si.render_device(scene, films["gaussian_r2"], smp, px.data_ptr(), stream)),
               ("filtered_sinc_r4", lambda: FL.render_filtered_torch(scene, cam, films["sinc_r4"], integ, smp, sinc, px))]
    for name, fn in runs_of:
        fn()                                                                  # warm-up (buffers, tile list, accumulators)
        runs = []
        for _ in range(a.reps):
            px.zero_()
            runs.append(fn())
        torch.cuda.synchronize()
        k = sorted(r["kernel_ms"] for r in runs)
        out[name] = {"kernel_ms": [round(r["kernel_ms"], 3) for r in runs], "median_kernel_ms": round(k[len(k) // 2], 3),
                     "trace_ms": [round(r["trace_ms"], 3) for r in runs], "camera_samples": runs[-1]["camera_samples"],
                     "trace_launches": runs[-1]["trace_launches"]}
        print("%s: %s" % (name, json.dumps(out[name])), flush=True)
    base = out["beauty"]["median_kernel_ms"]
    for name in ("filtered_gaussian_r2", "filtered_sinc_r4", "beauty_box_r2"):
        out[name]["overhead_ms"] = round(out[name]["median_kernel_ms"] - base, 3)
        out[name]["overhead_fraction"] = round(out[name]["overhead_ms"] / base, 4)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
