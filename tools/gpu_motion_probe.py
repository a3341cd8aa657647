"""Time of the previous-position pass (ftn_render_motion_device) next to the first-hit G-buffer pass (ftn_render_gbuffer_device) on the
same scene, samples and film, both into device buffers:
  python tools/gpu_motion_probe.py [--res 1024] [--spp 16] [--reps 5] [--out profiles/motion/probe.json]
Two scenes: the Cornell box with two of its three spheres moved through their transforms, and the rounded cube on its ground against a
copy whose vertices moved (triangles only).  kernel_ms is the whole call (HIP events on its stream), trace_ms the closest-hit launches
inside it; median_wall_ms is the call as the host sees it, which for the pass also holds the two scenes' correspondence check and the
upload of the remap table."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cornell_pair(be, res, create=True):
    from fountain_amd import Transform, scenes
    out = []
    for frame in (1, 0):
        b, cam, r = scenes.cornell(be, res=res)
        if frame == 0:                                   # the previous frame: the first sphere stood elsewhere, the second was squashed
            for k, t in ((0, Transform.translate(be, (-0.35, 0.3, -0.6))), (1, Transform.translate(be, (0.45, 0.1, -0.6)) * Transform.scale(be, 1.0, 0.8, 1.2))):
                b.spheres[k].object_to_world, b.spheres[k].world_to_object = t.raw, t.inverse().raw
        out.append(b.create_scene() if create else b)
    return out[0], out[1], cam, r


def cube_pair(be, res):
    import numpy as np
    from fountain_amd import PerspectiveCamera, SceneBuilder, scenes
    P, N, F = scenes.rounded_cube_mesh()
    made = []
    for frame in (1, 0):
        b = SceneBuilder(be)
        b.light_source("infinite", L=(0.5, 0.5, 0.5))
        b.material("matte", Kd=(0.5, 0.5, 0.5))
        scenes._quad(b, (-60, -60, -9.99), (60, -60, -9.99), (60, 60, -9.99), (-60, 60, -9.99))
        b.material("matte", Kd=(0.7, 0.5, 0.3))
        b.shape("trianglemesh", P=np.asarray(P, np.float32) * (1.0 if frame else 0.9), N=N, indices=F)
        made.append(b.create_scene())
    cam = PerspectiveCamera.look_at(be, (28, -28, 14), (0, 0, -2), (0, 0, 1), (res, res), fov=40.0)
    return made[0], made[1], cam, (res, res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion", "probe.json"))
    a = ap.parse_args()
    import torch
    from fountain_amd import Film, RandomSampler, default_backend
    from fountain_amd import gbuffer as G
    from fountain_amd import motion as M
    be = default_backend()
    out = {"res": a.res, "spp": a.spp, "reps": a.reps}
    for name, make in (("cornell", cornell_pair), ("rounded_cube", cube_pair)):
        scene, prev, cam, res = make(be, a.res)
        film = Film(be, res)
        smp = RandomSampler(a.spp, 0, indexed=True)
        gb = torch.zeros((film.height, film.width, 12), dtype=torch.float32, device="cuda:0")
        mv = torch.zeros((film.height, film.width, 8), dtype=torch.float32, device="cuda:0")
        G.render_gbuffer_torch(scene, cam, film, smp, gb)                     # warm-up (buffers, tile list)
        M.render_motion_torch(scene, prev, cam, film, smp, mv)
        rows = {}
        for what, run in (("gbuffer", lambda: G.render_gbuffer_torch(scene, cam, film, smp, gb)), ("motion", lambda: M.render_motion_torch(scene, prev, cam, film, smp, mv))):
            runs, wall = [], []
            for _ in range(a.reps):
                gb.zero_(); mv.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                runs.append(run())
                wall.append((time.perf_counter() - t0) * 1e3)
            k = sorted(r["kernel_ms"] for r in runs)
            rows[what] = {"kernel_ms": [round(r["kernel_ms"], 3) for r in runs], "trace_ms": [round(r["trace_ms"], 3) for r in runs],
                          "median_kernel_ms": round(k[len(k) // 2], 3), "median_wall_ms": round(sorted(wall)[len(wall) // 2], 3),
                          "rays_closest": runs[-1]["rays_closest"], "camera_samples": runs[-1]["camera_samples"]}
            print("%s %s: %s" % (name, what, json.dumps(rows[what])), flush=True)
        rows["n_prims"] = scene.info()["n_prims"]
        rows["motion_over_gbuffer"] = round(rows["motion"]["median_kernel_ms"] / rows["gbuffer"]["median_kernel_ms"], 4)
        out[name] = rows
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps({k: v["motion_over_gbuffer"] for k, v in out.items() if isinstance(v, dict)}))


if __name__ == "__main__":
    main()
