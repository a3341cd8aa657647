"""Time of the a-trous denoiser (ftn_denoise_device through denoise_torch) on the config-5 scene at 4 spp, next to the beauty step and
the G-buffer pass of the same run, all into device buffers:
  python tools/gpu_denoise_probe.py [--res 4096] [--reps 3] [--out profiles/denoise/probe.json]
Each denoiser time is one call bracketed by HIP events on the current stream (prepare + the levels' launches), median of --reps after a
warm-up; the per-kernel split comes from a separate `rocprofv3 --kernel-trace --stats` run of this script."""
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
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise", "probe.json"))
    a = ap.parse_args()
    import torch
    from fountain_amd import Film, PathIntegrator, RandomSampler, SamplerIntegrator, default_backend, film_resolve_device, scenes
    from fountain_amd import denoise as D
    from fountain_amd import gbuffer as G
    be = default_backend()
    t0 = time.time()
    b, cam, res = scenes.instanced_cubes(be, n_copies=a.copies, res=(a.res, a.res))
    scene = b.create_scene()
    film = Film(be, res)
    h, w = film.height, film.width
    out = {"scene": "config 5: %d copies of rounded_cube, %dx%d film, %d spp" % (a.copies, w, h, a.spp), "scene_build_s": round(time.time() - t0, 1),
           "reps": a.reps}
    med = lambda xs: sorted(xs)[len(xs) // 2]
    stream = torch.cuda.current_stream().cuda_stream
    smp = RandomSampler(a.spp, 0, indexed=True)

    px = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    si = SamplerIntegrator(cam, PathIntegrator(5, 1.0))
    si.render_device(scene, film, smp, px.data_ptr(), stream)                         # warm-up
    runs = []
    for _ in range(a.reps):
        px.zero_()
        runs.append(si.render_device(scene, film, smp, px.data_ptr(), stream)["kernel_ms"])
    out["beauty_ms"] = {"runs": [round(x, 3) for x in runs], "median": round(med(runs), 3)}
    rgb = torch.empty((h, w, 3), dtype=torch.float32, device="cuda:0")
    film_resolve_device(be, px.data_ptr(), w * h, rgb.data_ptr(), stream)

    raw = torch.zeros((h, w, 12), dtype=torch.float32, device="cuda:0")
    G.render_gbuffer_torch(scene, cam, film, smp, raw)                                # warm-up
    runs = []
    for _ in range(a.reps):
        raw.zero_()
        runs.append(G.render_gbuffer_torch(scene, cam, film, smp, raw)["kernel_ms"])
    out["gbuffer_ms"] = {"runs": [round(x, 3) for x in runs], "median": round(med(runs), 3)}
    gb = torch.empty_like(raw)
    G.resolve_torch(be, raw, gb)
    torch.cuda.synchronize()
    out["coverage_mean"] = round(float(gb[..., 10].mean()), 4)
    print("beauty %s, G-buffer %s" % (out["beauty_ms"], out["gbuffer_ms"]), flush=True)

    dst = torch.empty_like(rgb)
    ws = torch.empty(D.workspace_bytes(be, w, h), dtype=torch.uint8, device="cuda:0")
    out["workspace_bytes"] = ws.numel()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for levels in (1, 3, 5):
        p = D.default_params(be, levels=levels)
        D.denoise_torch(be, rgb, gb, dst, workspace=ws, params=p)                    # warm-up
        torch.cuda.synchronize()
        runs = []
        for _ in range(a.reps):
            ev0.record()
            D.denoise_torch(be, rgb, gb, dst, workspace=ws, params=p)
            ev1.record()
            ev1.synchronize()
            runs.append(ev0.elapsed_time(ev1))
        out["denoise_%d_levels_ms" % levels] = {"runs": [round(x, 3) for x in runs], "median": round(med(runs), 3)}
        print("denoise %d levels: %s" % (levels, out["denoise_%d_levels_ms" % levels]), flush=True)
    out["denoise_5_levels_over_beauty"] = round(out["denoise_5_levels_ms"]["median"] / out["beauty_ms"]["median"], 4)
    out["denoise_5_levels_over_gbuffer"] = round(out["denoise_5_levels_ms"]["median"] / out["gbuffer_ms"]["median"], 4)
    out["finite_output"] = bool(torch.isfinite(dst).all())
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
