"""Time and tuning of the variance-guided a-trous denoiser (include/fountain_hip_denoise_guided.h).

  python tools/gpu_denoise_guided_probe.py [--res 4096] [--reps 3] [--out profiles/denoise_guided/probe.json]
      config-5 scene at 4 spp: beauty and moments (render_moments_torch), G-buffer, then ftn_denoise_guided_device and ftn_denoise_device
      at 1, 3 and 5 levels in the same run, each call bracketed by HIP events on the current stream, median of --reps after a warm-up.
      The per-kernel split comes from a separate `rocprofv3 --kernel-trace --stats` run of this script.
  python tools/gpu_denoise_guided_probe.py --save-inputs FILE.npz
      renders the sweep's inputs on the GPU once: for each test scene, beauty, G-buffer and variance at 4 spp and a 1024-spp reference
  python tools/gpu_denoise_guided_probe.py --sweep FILE.npz [--sweep-out profiles/denoise_guided/sweep.json]
      the parameter sweep on those inputs with the host twin (no GPU): relative MSE against the reference for each grid point, and
      ftn_denoise at its defaults beside it
"""
import argparse
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GRID = dict(sigma_variance=[1.0, 2.0, 4.0, 8.0], rel_eps=[0.0, 1e-4, 1e-2], sigma_plane=[1e-4, 1e-2, 0.1])


def rel_mse(img, ref):
    import numpy as np
    return float(np.mean(((img.astype(np.float64) - ref) / (ref + 1e-2)) ** 2))


def save_inputs(path):
    import numpy as np
    from fountain_amd import PathIntegrator, RandomSampler, default_backend, scenes
    import test_denoise as TD
    import test_denoise_guided as TG
    be = default_backend()
    makes = {"cornell": lambda b: scenes.cornell(b, res=128), "yard": TD._yard, "split_room": TG.split_room}
    out = {}
    for name, make in makes.items():
        rgb, gb, var4 = TG.rendered(be, make, 4)
        b, cam, res = make(be)
        ref, _, _, _ = scenes.render(be, b, cam, res, PathIntegrator(5, 1.0), RandomSampler(1024, 77, indexed=True))
        out.update({name + "_rgb": rgb, name + "_gb": gb, name + "_var4": var4, name + "_ref": ref})
        print("%s: %r, relative MSE of the 4-spp image %.5g" % (name, rgb.shape, rel_mse(rgb, ref)), flush=True)
    np.savez_compressed(path, **out)


def sweep(path, out_path):
    import numpy as np
    from fountain_amd import default_backend
    from fountain_amd import denoise as D
    be = default_backend()
    d = np.load(path)
    names = sorted(k[:-4] for k in d.files if k.endswith("_rgb"))
    res = {"inputs": "4 spp beauty, G-buffer and variance against 1024 spp, rendered on the GPU by --save-inputs; filtered by the host twin",
           "metric": "mean(((out - ref) / (ref + 0.01))^2)", "scenes": {}}
    for n in names:
        rgb, gb, var4, ref = d[n + "_rgb"], d[n + "_gb"], d[n + "_var4"], d[n + "_ref"]
        res["scenes"][n] = {"noisy": rel_mse(rgb, ref), "unguided_defaults": rel_mse(D.denoise_cpu(be, rgb, gb), ref)}
    rows = []
    for sv, re, sp in itertools.product(GRID["sigma_variance"], GRID["rel_eps"], GRID["sigma_plane"]):
        row = dict(sigma_variance=sv, rel_eps=re, sigma_plane=sp)
        for n in names:
            out = D.denoise_guided_cpu(be, d[n + "_rgb"], d[n + "_gb"], d[n + "_var4"], dict(sigma_variance=sv, rel_eps=re, sigma_plane=sp))
            row[n] = rel_mse(out, d[n + "_ref"])
        # the score: the mean over the scenes of the error relative to the unguided filter at its defaults
        row["score"] = float(np.mean([row[n] / res["scenes"][n]["unguided_defaults"] for n in names]))
        rows.append(row)
        print(json.dumps(row), flush=True)
    rows.sort(key=lambda r: r["score"])
    res["grid"] = GRID
    res["rows_by_score"] = rows
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("best: %s" % json.dumps(rows[0]))


def probe(a):
    import torch
    from fountain_amd import Film, PathIntegrator, RandomSampler, SamplerIntegrator, default_backend, film_resolve_device, scenes
    from fountain_amd import denoise as D
    from fountain_amd import gbuffer as G
    from fountain_amd import moments as M
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
    si = SamplerIntegrator(cam, PathIntegrator(5, 1.0))
    px = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    mom = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    M.render_moments_torch(scene, cam, film, si.radiance, smp, px, mom)
    rgb = torch.empty((h, w, 3), dtype=torch.float32, device="cuda:0")
    film_resolve_device(be, px.data_ptr(), w * h, rgb.data_ptr(), stream)
    var4 = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
    M.resolve_torch(be, px, mom, var4)
    raw = torch.zeros((h, w, 12), dtype=torch.float32, device="cuda:0")
    G.render_gbuffer_torch(scene, cam, film, smp, raw)
    gb = torch.empty_like(raw)
    G.resolve_torch(be, raw, gb)
    torch.cuda.synchronize()
    out["coverage_mean"] = round(float(gb[..., 10].mean()), 4)
    out["variance_finite_fraction"] = round(float(torch.isfinite(var4[..., :3]).all(-1).float().mean()), 4)

    dst = torch.empty_like(rgb)
    ws = torch.empty(D.guided_workspace_bytes(be, w, h), dtype=torch.uint8, device="cuda:0")
    out["workspace_bytes"] = ws.numel()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(call):
        call()                                                                       # warm-up
        torch.cuda.synchronize()
        runs = []
        for _ in range(a.reps):
            ev0.record()
            call()
            ev1.record()
            ev1.synchronize()
            runs.append(ev0.elapsed_time(ev1))
        return {"runs": [round(x, 3) for x in runs], "median": round(med(runs), 3)}

    for levels in (1, 3, 5):
        pg, pu = D.guided_params(be, levels=levels), D.default_params(be, levels=levels)
        out["guided_%d_levels_ms" % levels] = timed(lambda: D.denoise_guided_torch(be, rgb, gb, var4, dst, workspace=ws, params=pg))
        out["unguided_%d_levels_ms" % levels] = timed(lambda: D.denoise_torch(be, rgb, gb, dst, workspace=ws, params=pu))
        out["guided_over_unguided_%d_levels" % levels] = round(out["guided_%d_levels_ms" % levels]["median"] /
                                                               out["unguided_%d_levels_ms" % levels]["median"], 4)
        print("%d levels: guided %s, unguided %s" % (levels, out["guided_%d_levels_ms" % levels], out["unguided_%d_levels_ms" % levels]), flush=True)
    D.denoise_guided_torch(be, rgb, gb, var4, dst, workspace=ws)
    torch.cuda.synchronize()
    out["finite_output"] = bool(torch.isfinite(dst).all())
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=4096)
    ap.add_argument("--copies", type=int, default=2309)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_guided", "probe.json"))
    ap.add_argument("--save-inputs", default=None)
    ap.add_argument("--sweep", default=None)
    ap.add_argument("--sweep-out", default=os.path.join(ROOT, "profiles", "denoise_guided", "sweep.json"))
    a = ap.parse_args()
    if a.save_inputs:
        save_inputs(a.save_inputs)
    elif a.sweep:
        sweep(a.sweep, a.sweep_out)
    else:
        probe(a)


if __name__ == "__main__":
    main()
