"""Time and tuning of temporal reprojection and accumulation (include/fountain_hip_temporal.h).

  python tools/gpu_temporal_probe.py [--res 4096] [--reps 5] [--out profiles/temporal/probe.json]
      config-5 scene at 4 spp: beauty and moments (render_moments_torch), G-buffer, then ftn_temporal_accumulate_device (a first frame,
      and a frame that reprojects into the history of a camera moved by a few pixels) and a 5-level ftn_denoise_guided_device in the same
      run, each call bracketed by HIP events on the current stream, median of --reps after a warm-up.
  python tools/gpu_temporal_probe.py --save-inputs FILE.npz
      renders the sweep's inputs on the GPU once: the moving view of tests/test_temporal.py (Cornell 128^2, eight cameras on a short arc,
      4 spp each: beauty, G-buffer, variance, the cameras) and the 1024-spp reference at the last camera
  python tools/gpu_temporal_probe.py --sweep FILE.npz [--sweep-out profiles/temporal/sweep.json]
      the parameter sweep on those inputs with the host twins (no GPU): for each grid point, the relative MSE of the guided filter over the
      accumulated last frame against the reference, and its ratio to the guided filter over the last frame alone
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

GRID = dict(alpha_min=[0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6], normal_tol=[0.01, 0.1, 1.0], plane_tol=[0.001, 0.01, 0.1], albedo_tol=[0.0, 0.01, 0.05, 0.2, 1.0])


def rel_mse(img, ref):
    import numpy as np
    return float(np.mean(((img.astype(np.float64) - ref) / (ref + 1e-2)) ** 2))


def save_inputs(path):
    import numpy as np
    from fountain_amd import PathIntegrator, RandomSampler, default_backend, scenes
    import test_temporal as TT
    be = default_backend()
    b, cam, res = scenes.cornell(be, res=128)
    scene = b.create_scene()
    cams = [TT.arc_camera(be, k) for k in range(8)]
    out = {}
    for k, c in enumerate(cams):
        rgb, gb, var4, film = TT.render_frame(be, scene, c, res, RandomSampler(4, 100 + k, indexed=True))
        out.update({"rgb_%d" % k: rgb, "gb_%d" % k: gb, "var4_%d" % k: var4, "camera_%d" % k: np.frombuffer(bytes(c.desc), np.uint8)})
        out["film"] = np.frombuffer(bytes(film.desc), np.uint8)
    ref, _, _, _ = scenes.render(be, None, cam, res, PathIntegrator(5, 1.0), RandomSampler(1024, 77, indexed=True), scene=scene)
    out["ref"] = ref
    print("moving view: 8 frames of %r, relative MSE of the last 4-spp frame %.5g" % (ref.shape, rel_mse(out["rgb_7"], ref)), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **out)


def sweep(path, out_path):
    import numpy as np
    from fountain_amd import _abi as A, default_backend
    from fountain_amd import denoise as D
    from fountain_amd import temporal as T
    be = default_backend()
    d = np.load(path)
    n = len([k for k in d.files if k.startswith("rgb_")])
    cams = [A.ftn_camera_desc.from_buffer_copy(d["camera_%d" % k].tobytes()) for k in range(n)]
    film = A.ftn_film_desc.from_buffer_copy(d["film"].tobytes())
    frames = [(d["rgb_%d" % k], d["gb_%d" % k], d["var4_%d" % k]) for k in range(n)]
    ref = d["ref"]
    last = frames[-1]
    alone = rel_mse(D.denoise_guided_cpu(be, *last), ref)
    res = {"inputs": "Cornell 128^2, %d cameras on a short arc, 4 spp each, against 1024 spp at the last camera, rendered on the GPU by --save-inputs; "
                     "accumulated and filtered by the host twins" % n,
           "metric": "mean(((out - ref) / (ref + 0.01))^2) of ftn_denoise_guided (defaults) over the accumulated last frame; ratio = that over "
                     "the same filter on the last frame alone",
           "noisy_last_frame": rel_mse(last[0], ref), "guided_alone": alone}
    rows = []
    for am, nt, pt, at in itertools.product(GRID["alpha_min"], GRID["normal_tol"], GRID["plane_tol"], GRID["albedo_tol"]):
        acc = T.TemporalAccumulator(be, dict(alpha_min=am, normal_tol=nt, plane_tol=pt, albedo_tol=at), cpu=True)
        for f, c in zip(frames, cams):
            out, ovar = acc.push(f[0], f[1], f[2], c, film)
        both = rel_mse(D.denoise_guided_cpu(be, out, last[1], ovar), ref)
        row = dict(alpha_min=am, normal_tol=nt, plane_tol=pt, albedo_tol=at, accumulated=rel_mse(out, ref), accumulated_guided=both, ratio=both / alone,
                   mean_history=float(acc.history[..., 3].mean()))
        rows.append(row)
        print(json.dumps(row), flush=True)
    rows.sort(key=lambda r: r["ratio"])
    res["grid"] = GRID
    res["rows_by_ratio"] = rows
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("best: %s" % json.dumps(rows[0]))


def probe(a):
    import numpy as np
    import torch
    from fountain_amd import Film, PathIntegrator, PerspectiveCamera, RandomSampler, SamplerIntegrator, default_backend, film_resolve_device, scenes
    from fountain_amd import denoise as D
    from fountain_amd import gbuffer as G
    from fountain_amd import moments as M
    from fountain_amd import temporal as T
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
    dev = "cuda:0"
    px = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
    mom = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
    M.render_moments_torch(scene, cam, film, si.radiance, smp, px, mom)
    rgb = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    film_resolve_device(be, px.data_ptr(), w * h, rgb.data_ptr(), stream)
    var4 = torch.empty((h, w, 4), dtype=torch.float32, device=dev)
    M.resolve_torch(be, px, mom, var4)
    raw = torch.zeros((h, w, 12), dtype=torch.float32, device=dev)
    G.render_gbuffer_torch(scene, cam, film, smp, raw)
    gb = torch.empty_like(raw)
    G.resolve_torch(be, raw, gb)
    torch.cuda.synchronize()
    del px, mom, raw
    out["coverage_mean"] = round(float(gb[..., 10].mean()), 4)

    # the previous camera: the scene's own, its eye moved sideways by 0.1 % of its distance (a few pixels at 4096^2); the static scene's
    # G-buffer serves both frames
    side = int(np.ceil(a.copies ** (1.0 / 3.0)))
    ext = 0.5 * side * 26.0
    eye = np.array((1.9 * ext, -2.3 * ext, 1.4 * ext))
    moved = eye + 1e-3 * np.linalg.norm(eye) * np.array((2.3, 1.9, 0.0)) / np.hypot(2.3, 1.9)
    prev_cam = PerspectiveCamera.look_at(be, tuple(moved), (0, 0, 0), (0, 0, 1), res, fov=38.0, focal_dist=float(np.linalg.norm(eye)))
    hist = [torch.empty((h, w, 8), dtype=torch.float32, device=dev) for _ in range(2)]
    acc_rgb, acc_var = torch.empty_like(rgb), torch.empty_like(var4)
    dst = torch.empty_like(rgb)
    ws = torch.empty(D.guided_workspace_bytes(be, w, h), dtype=torch.uint8, device=dev)
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

    out["temporal_first_frame_ms"] = timed(lambda: T.temporal_accumulate_torch(be, rgb, gb, var4, prev_cam, film, hist[0], acc_rgb, acc_var))
    out["temporal_reprojected_ms"] = timed(lambda: T.temporal_accumulate_torch(be, rgb, gb, var4, cam, film, hist[1], acc_rgb, acc_var,
                                                                               prev=(prev_cam, gb, hist[0])))
    out["temporal_static_ms"] = timed(lambda: T.temporal_accumulate_torch(be, rgb, gb, var4, prev_cam, film, hist[1], acc_rgb, acc_var,
                                                                          prev=(prev_cam, gb, hist[0])))
    T.temporal_accumulate_torch(be, rgb, gb, var4, cam, film, hist[1], acc_rgb, acc_var, prev=(prev_cam, gb, hist[0]))
    torch.cuda.synchronize()
    out["history_found_fraction"] = round(float((hist[1][..., 3] > 1).float().mean()), 4)
    out["guided_5_levels_ms"] = timed(lambda: D.denoise_guided_torch(be, acc_rgb, gb, acc_var, dst, workspace=ws))
    out["temporal_over_guided_5_levels"] = round(out["temporal_reprojected_ms"]["median"] / out["guided_5_levels_ms"]["median"], 4)
    # bytes a reprojected pixel moves when every tap counts: reads rgb 12, gb12 48, var4 16, four taps of history 4 x 32 and of the previous
    # G-buffer's normal, position, depth and coverage 4 x 32; writes history 32, rgb 12, var4 16
    out["bytes_per_pixel_upper"] = 12 + 48 + 16 + 4 * 32 + 4 * 32 + 32 + 12 + 16
    out["effective_GB_per_s_upper"] = round(out["bytes_per_pixel_upper"] * w * h / (out["temporal_reprojected_ms"]["median"] * 1e-3) / 1e9, 1)
    out["finite_output"] = bool(torch.isfinite(acc_rgb).all())
    for k in ("temporal_first_frame_ms", "temporal_reprojected_ms", "temporal_static_ms", "guided_5_levels_ms"):
        print("%s: %s" % (k, out[k]), flush=True)
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal", "probe.json"))
    ap.add_argument("--save-inputs", default=None)
    ap.add_argument("--sweep", default=None)
    ap.add_argument("--sweep-out", default=os.path.join(ROOT, "profiles", "temporal", "sweep.json"))
    a = ap.parse_args()
    if a.save_inputs:
        save_inputs(a.save_inputs)
    elif a.sweep:
        sweep(a.sweep, a.sweep_out)
    else:
        probe(a)


if __name__ == "__main__":
    main()
