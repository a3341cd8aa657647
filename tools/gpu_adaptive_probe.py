"""Cost and benefit of per-tile adaptive sampling (ftn_render_adaptive_device) against uniform moments renders (ftn_render_moments_device),
both into device buffers, PathIntegrator(5, 1.0), medians of --reps calls (kernel_ms: HIP events around the whole call):
  python tools/gpu_adaptive_probe.py [--res 4096] [--spp 64] [--reps 3] [--small-res 256] [--skip-config5] [--out profiles/adaptive/probe.json]
config5: the config-5 scene at --res, adaptive (defaults) against uniform at N = --spp; rounds, camera samples, and per round the part of
the call outside the wavefront's kernel groups (kernel_ms - trace - any-hit - shade - sort, against the same quantity of the uniform call).
small: a sphere on a floor under a black sky at --small-res, relative MSE against 1024 spp, adaptive against uniform renders at equal or
less time.  --sweep: thresholds 0.02 .. 0.4 on the Cornell box and the small scene, relative MSE against uniform at equal samples."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sphere_on_black(be, res):
    from fountain_amd import PerspectiveCamera, SceneBuilder, scenes
    b = SceneBuilder(be)
    b.attribute_begin(); b.material("matte", Kd=(0.0, 0.0, 0.0)); b.area_light_source("diffuse", L=(30.0, 30.0, 30.0))
    b.translate((1.6, 0.5, 2.2)); b.shape("sphere", radius=0.25); b.attribute_end()
    b.attribute_begin(); b.material("matte", Kd=(0.7, 0.55, 0.4)); b.translate((-0.4, 0.0, 0.0)); b.shape("sphere", radius=0.8); b.attribute_end()
    b.attribute_begin(); b.material("matte", Kd=(0.5, 0.5, 0.5))
    scenes._quad(b, (-6, -6, -0.8), (6, -6, -0.8), (6, 6, -0.8), (-6, 6, -0.8)); b.attribute_end()
    cam = PerspectiveCamera.look_at(be, (0.0, -5.0, 0.3), (0.0, 0.0, 0.3), (0, 0, 1), (res, res), fov=50.0)
    return b, cam, (res, res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=4096)
    ap.add_argument("--copies", type=int, default=2309)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small-res", type=int, default=256)
    ap.add_argument("--skip-config5", action="store_true")
    ap.add_argument("--skip-small", action="store_true")
    ap.add_argument("--sweep", action="store_true", help="only the threshold sweep behind the defaults (Cornell box and the small scene)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive", "probe.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from fountain_amd import Film, PathIntegrator, RandomSampler, default_backend, scenes
    from fountain_amd import adaptive as AD
    from fountain_amd import moments as M
    be = default_backend()
    integ = PathIntegrator(5, 1.0)
    out = {"reps": a.reps}

    def bufs(film):
        px = torch.zeros((film.height, film.width, 4), dtype=torch.float32, device="cuda:0")
        return px, torch.zeros_like(px), torch.zeros((film.height, film.width), dtype=torch.int32, device="cuda:0")

    def median_runs(fn, reset):
        fn()                                                              # warm-up (buffers, wavefront, moment accumulators)
        runs = []
        for _ in range(a.reps):
            reset()
            runs.append(fn())
        torch.cuda.synchronize()
        return runs, sorted(r[-1]["kernel_ms"] for r in runs)[len(runs) // 2]

    def outside(st):
        return st["kernel_ms"] - st["trace_ms"] - st["any_ms"] - st["shade_ms"] - st["sort_ms"]

    def rgb(p):
        import ctypes as C
        img = np.zeros(p.shape[:-1] + (3,), np.float32)
        be.lib.ftn_film_resolve(np.ascontiguousarray(p, np.float32).ctypes.data_as(C.c_void_p), C.c_size_t(p.size // 4), img.ctypes.data_as(C.c_void_p))
        return img.astype(np.float64)

    if a.sweep:
        # the threshold against the relative MSE at 1024 spp and the samples spent, with a uniform render of at least as many samples
        out["sweep"] = {}
        for name, make in (("cornell", lambda: scenes.cornell(be, res=a.small_res)), ("sphere_on_black", lambda: sphere_on_black(be, a.small_res))):
            b, cam, res = make()
            scene = b.create_scene()
            film = Film(be, res)
            px, mo, cnt = bufs(film)
            M.render_moments_torch(scene, cam, film, integ, RandomSampler(1024, 1000, indexed=True), px, mo)
            ref = rgb(px.cpu().numpy())
            rel = lambda p: float((((rgb(p) - ref) ** 2) / (ref * ref + 1e-2)).mean())
            rows = []
            for t in (0.02, 0.05, 0.1, 0.2, 0.4):
                px.zero_(); mo.zero_()
                info, st = AD.render_adaptive_torch(scene, cam, film, integ, RandomSampler(a.spp, 0, indexed=True), AD.params(be, threshold=t), px, mo, cnt)
                e_a = rel(px.cpu().numpy())
                spp = -(-int(st["camera_samples"]) // (film.width * film.height))
                px.zero_(); mo.zero_()
                M.render_moments_torch(scene, cam, film, integ, RandomSampler(spp, 0, indexed=True), px, mo)
                e_u = rel(px.cpu().numpy())
                rows.append({"t": t, "rounds": info["rounds"], "spp_mean": round(st["camera_samples"] / (film.width * film.height), 2),
                             "tiles_at_max": info["tiles_at_max"], "tiles": info["tiles"], "rel_mse": e_a, "uniform_spp": spp, "uniform_rel_mse": e_u,
                             "mse_ratio": round(e_a / e_u, 3)})
                print("%s %s" % (name, json.dumps(rows[-1])), flush=True)
            out["sweep"][name] = {"N": a.spp, "res": res[0], "rows": rows}
        a.skip_config5 = a.skip_small = True

    if not a.skip_config5:
        t0 = time.time()
        b, cam, res = scenes.instanced_cubes(be, n_copies=a.copies, res=(a.res, a.res))
        scene = b.create_scene()
        film = Film(be, res)
        px, mo, cnt = bufs(film)
        reset = lambda: (px.zero_(), mo.zero_())
        c5 = {"scene": "config 5: %d copies of rounded_cube, %dx%d film, N = %d" % (a.copies, a.res, a.res, a.spp), "scene_build_s": round(time.time() - t0, 1)}
        smp = RandomSampler(a.spp, 0, indexed=True)
        u_runs, u_ms = median_runs(lambda: (M.render_moments_torch(scene, cam, film, integ, smp, px, mo),), reset)
        prm = AD.params(be)
        a_runs, a_ms = median_runs(lambda: AD.render_adaptive_torch(scene, cam, film, integ, smp, prm, px, mo, cnt), reset)
        info, st = a_runs[-1]
        ust = u_runs[-1][0]
        counts = cnt.cpu().numpy()
        c5["uniform"] = {"kernel_ms": [round(r[0]["kernel_ms"], 2) for r in u_runs], "median_ms": round(u_ms, 2), "camera_samples": ust["camera_samples"],
                         "outside_groups_ms": round(outside(ust), 2), "trace_launches": ust["trace_launches"]}
        c5["adaptive"] = {"params": {k: getattr(prm, k) for k, _ in prm._fields_}, "kernel_ms": [round(r[1]["kernel_ms"], 2) for r in a_runs],
                          "median_ms": round(a_ms, 2), "info": info, "camera_samples": st["camera_samples"], "trace_launches": st["trace_launches"],
                          "outside_groups_ms": round(outside(st), 2), "tiles_per_count": {int(n): int((counts[::16, ::16] == n).sum()) for n in np.unique(counts)}}
        c5["speedup"] = round(u_ms / a_ms, 3)
        c5["samples_ratio"] = round(st["camera_samples"] / ust["camera_samples"], 4)
        c5["outside_groups_per_round_ms"] = round((outside(st) - outside(ust)) / max(1, info["rounds"]), 2)
        out["config5"] = c5
        print("config5: %s" % json.dumps(c5), flush=True)
        del scene, px, mo, cnt
        torch.cuda.synchronize()

    if not a.skip_small:
        b, cam, res = sphere_on_black(be, a.small_res)
        scene = b.create_scene()
        film = Film(be, res)
        px, mo, cnt = bufs(film)
        reset = lambda: (px.zero_(), mo.zero_())

        M.render_moments_torch(scene, cam, film, integ, RandomSampler(1024, 1000, indexed=True), px, mo)
        ref = rgb(px.cpu().numpy())

        def rel_mse(p):
            return float((((rgb(p) - ref) ** 2) / (ref * ref + 1e-2)).mean())
        sm = {"scene": "sphere and floor under a black sky, %dx%d, reference 1024 spp" % res, "uniform": {}}
        prm = AD.params(be)
        a_runs, a_ms = median_runs(lambda: AD.render_adaptive_torch(scene, cam, film, integ, RandomSampler(a.spp, 0, indexed=True), prm, px, mo, cnt), reset)
        sm["adaptive"] = {"N": a.spp, "median_ms": round(a_ms, 3), "info": a_runs[-1][0], "rel_mse": rel_mse(px.cpu().numpy()),
                          "spp_mean": round(float(cnt.float().mean()), 2)}
        for spp in sorted({4, 8, 12, 16, 24, 32, 48, a.spp}):
            runs, ms = median_runs(lambda: (M.render_moments_torch(scene, cam, film, integ, RandomSampler(spp, 0, indexed=True), px, mo),), reset)
            sm["uniform"][spp] = {"median_ms": round(ms, 3), "rel_mse": rel_mse(px.cpu().numpy())}
        fit = [s for s, v in sm["uniform"].items() if v["median_ms"] <= a_ms]
        sm["uniform_at_equal_time"] = max(fit) if fit else None
        if fit:
            sm["mse_ratio_at_equal_time"] = round(sm["adaptive"]["rel_mse"] / sm["uniform"][max(fit)]["rel_mse"], 3)
        out["small"] = sm
        print("small: %s" % json.dumps(sm), flush=True)

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
