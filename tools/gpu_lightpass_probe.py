"""Time of the light-group pass (ftn_render_lightpass_device, all lights) next to the ambient-occlusion pass at one ray per surface
(ftn_render_ao_device, rays = 1) and the first-hit G-buffer pass (ftn_render_gbuffer_device) on the same scene, samples and film, all
into device buffers:
  python tools/gpu_lightpass_probe.py [--res 1024] [--spp 16] [--reps 5] [--out profiles/lightpass/probe.json]
The two scenes of tools/gpu_motion_probe.py: the Cornell box (spheres: the four-box any-hit kernel; its lights are the two triangles of
the ceiling quad) and the rounded cube on its ground under a uniform infinite light (triangles only: the eight-box kernel).  kernel_ms is
the whole call (HIP events on its stream), trace_ms the closest-hit launches and any_ms the any-hit launch inside it.  The question the
figures answer: does one shadow ray per surface cost about what one occlusion ray does?"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightpass", "probe.json"))
    a = ap.parse_args()
    import torch
    from gpu_motion_probe import cornell_pair, cube_pair
    from fountain_amd import Film, RandomSampler, default_backend
    from fountain_amd import ao as AO
    from fountain_amd import gbuffer as G
    from fountain_amd import lightpass as LP
    be = default_backend()
    out = {"res": a.res, "spp": a.spp, "reps": a.reps}
    for name, make in (("cornell", cornell_pair), ("rounded_cube", cube_pair)):
        scene, _, cam, res = make(be, a.res)
        film = Film(be, res)
        smp = RandomSampler(a.spp, 0, indexed=True)
        gb = torch.zeros((film.height, film.width, 12), dtype=torch.float32, device="cuda:0")
        px = torch.zeros((film.height, film.width, 8), dtype=torch.float32, device="cuda:0")
        passes = (("gbuffer", lambda: G.render_gbuffer_torch(scene, cam, film, smp, gb)), ("ao1", lambda: AO.render_ao_torch(scene, cam, film, smp, px, rays=1)),
                  ("lightpass", lambda: LP.render_lightpass_torch(scene, cam, film, smp, px)))
        for _, run in passes:                              # warm-up (buffers, tile list)
            run()
        rows = {}
        for what, run in passes:
            runs, wall = [], []
            for _ in range(a.reps):
                gb.zero_(); px.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                runs.append(run())
                wall.append((time.perf_counter() - t0) * 1e3)
            k = sorted(r["kernel_ms"] for r in runs)
            rows[what] = {"kernel_ms": [round(r["kernel_ms"], 3) for r in runs], "trace_ms": [round(r["trace_ms"], 3) for r in runs],
                          "any_ms": [round(r["any_ms"], 3) for r in runs],
                          "median_kernel_ms": round(k[len(k) // 2], 3), "median_wall_ms": round(sorted(wall)[len(wall) // 2], 3),
                          "rays_closest": runs[-1]["rays_closest"], "rays_any": runs[-1]["rays_any"], "camera_samples": runs[-1]["camera_samples"]}
            print("%s %s: %s" % (name, what, json.dumps(rows[what])), flush=True)
        rows["n_prims"], rows["n_lights"] = scene.info()["n_prims"], scene.info()["n_lights"]
        rows["lightpass_over_ao1"] = round(rows["lightpass"]["median_kernel_ms"] / rows["ao1"]["median_kernel_ms"], 4)
        rows["lightpass_over_gbuffer"] = round(rows["lightpass"]["median_kernel_ms"] / rows["gbuffer"]["median_kernel_ms"], 4)
        out[name] = rows
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps({k: [v["lightpass_over_ao1"], v["lightpass_over_gbuffer"]] for k, v in out.items() if isinstance(v, dict)}))


if __name__ == "__main__":
    main()
