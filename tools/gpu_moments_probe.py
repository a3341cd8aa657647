"""Cost of the second moments (ftn_render_moments_device) on the config-5 scene next to the beauty step alone (ftn_render_device), 16 spp,
PathIntegrator(5, 1.0), both into device buffers:
  python tools/gpu_moments_probe.py [--res 4096] [--reps 3] [--out profiles/moments/probe.json]
kernel_ms is the whole call (HIP events on its stream); the overhead is the difference of the medians."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moments", "probe.json"))
    a = ap.parse_args()
    import torch
    from fountain_amd import Film, PathIntegrator, RandomSampler, SamplerIntegrator, default_backend, scenes
    from fountain_amd import moments as M
    be = default_backend()
    t0 = time.time()
    b, cam, res = scenes.instanced_cubes(be, n_copies=a.copies, res=(a.res, a.res))
    scene = b.create_scene()
    film = Film(be, res)
    out = {"scene": "config 5: %d copies of rounded_cube, %dx%d film, %d spp" % (a.copies, a.res, a.res, a.spp), "scene_build_s": round(time.time() - t0, 1), "reps": a.reps}
    integ = PathIntegrator(5, 1.0)
    smp = RandomSampler(a.spp, 0, indexed=True)
    px = torch.zeros((film.height, film.width, 4), dtype=torch.float32, device="cuda:0")
    mo = torch.zeros_like(px)
    si = SamplerIntegrator(cam, integ)
    stream = torch.cuda.current_stream().cuda_stream

    def beauty():
        return si.render_device(scene, film, smp, px.data_ptr(), stream)

    def moments():
        mo.zero_()
        return M.render_moments_torch(scene, cam, film, integ, smp, px, mo)

    for name, fn in (("beauty", beauty), ("moments", moments)):
        fn()                                                                  # warm-up (buffers, tile list, moment accumulators)
        runs = []
        for _ in range(a.reps):
            px.zero_()
            runs.append(fn())
        torch.cuda.synchronize()
        k = sorted(r["kernel_ms"] for r in runs)
        out[name] = {"kernel_ms": [round(r["kernel_ms"], 3) for r in runs], "median_kernel_ms": round(k[len(k) // 2], 3),
                     "trace_ms": [round(r["trace_ms"], 3) for r in runs], "camera_samples": runs[-1]["camera_samples"],
                     "spill_samples": runs[-1]["spill_samples"], "trace_launches": runs[-1]["trace_launches"]}
        print("%s: %s" % (name, json.dumps(out[name])), flush=True)
    out["overhead_ms"] = round(out["moments"]["median_kernel_ms"] - out["beauty"]["median_kernel_ms"], 3)
    out["overhead_fraction"] = round(out["overhead_ms"] / out["beauty"]["median_kernel_ms"], 4)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
