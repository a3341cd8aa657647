"""Cost of the vector-blur stage (ftn_vectorblur_device) on device buffers:
  python tools/gpu_vectorblur_probe.py [--res 4096] [--reps 3] [--out profiles/vectorblur/probe.json] [--kernel-trace FILE.csv]
on a seeded image of --res squared under a rotational motion field (half velocities from 0 at the centre to the clamp of 16 pixels towards
the corners, so tiles of every blur length take part) with a two-layer G-buffer, and on the same image without motion (the tile-uniform
copy).  Each figure is the median of --reps calls timed with HIP events on the stream, after one warm-up call.  Beside each call stands the
time its bytes would take at the copy rate measured in the same session (a device-to-device copy of the image): the motion vectors and
the G-buffer's lines read once, the per-pixel records written once, and per pixel of a blurred tile the image and the records read once
more and the output written -- the taps themselves are counted as cache hits, which is the floor the gather is compared with.
A call launches its kernels back to back on one stream, so the time of each kernel comes from a kernel trace of this very program: run
it under `rocprofv3 --kernel-trace --output-format csv -- python tools/gpu_vectorblur_probe.py --trace-run`, then pass the trace's
*_kernel_trace.csv as --kernel-trace; the last --reps calls of the trace are reported per launch in launch order."""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAUNCHES = ("k_vb_velocity_tilemax", "k_vb_neighbour", "k_vb_gather")


def inputs(res, seed=1):
    import numpy as np
    rng = np.random.default_rng(seed)
    img = (rng.uniform(0.0, 2.0, (res, res, 3)) ** 2).astype(np.float32)
    ys, xs = np.mgrid[0:res, 0:res].astype(np.float32)
    c = 0.5 * (res - 1)
    k = np.float32(4.0 * 16.0 / (0.6 * res))                        # half velocity = 0.25 m reaches 16 pixels at 0.6 res from the centre
    motion = np.stack([-(ys - c) * k, (xs - c) * k], axis=-1).astype(np.float32)
    gb12 = np.zeros((res, res, 12), np.float32)
    gb12[..., 9] = np.where((xs // 96 + ys // 96) % 2 == 0, 2.0, 5.0)
    gb12[..., 10] = 1.0
    return img, motion, gb12


def call_bytes(n, blurred_share, with_gb):
    """bytes one call must move if every tap hit a cache: (per launch, in all)"""
    velocity = n * (8 + (48 if with_gb else 0) + 16)               # the G-buffer's two floats bring their whole 48-byte pixel
    gather = n * (12 + 12) + int(n * blurred_share) * 16
    return {"k_vb_velocity_tilemax": velocity, "k_vb_neighbour": 2 * 16 * (n // 256), "k_vb_gather": gather}, velocity + gather


def per_kernel(trace_csv, reps, nbytes):
    rows = [r for r in csv.DictReader(open(trace_csv)) if "k_vb_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    n = len(LAUNCHES)
    rows = rows[-reps * n:]
    assert len(rows) == reps * n, "the trace holds fewer vector-blur launches than --reps calls"
    out = []
    for i, what in enumerate(LAUNCHES):
        assert what in rows[i]["Kernel_Name"]
        us = [(int(rows[c * n + i]["End_Timestamp"]) - int(rows[c * n + i]["Start_Timestamp"])) / 1e3 for c in range(reps)]
        med = statistics.median(us)
        out.append({"kernel": rows[i]["Kernel_Name"].split("(")[0].replace("void ", "").replace("ftn::", ""), "us": [round(x, 2) for x in us],
                    "median_us": round(med, 2), "bytes": nbytes[what], "GB_per_s": round(nbytes[what] / med / 1e3, 1)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vectorblur", "probe.json"))
    ap.add_argument("--kernel-trace", default=None, help="the kernel trace (csv) of a --trace-run of this program")
    ap.add_argument("--trace-run", action="store_true", help="only the warm-up and --reps default calls; writes nothing")
    a = ap.parse_args()
    import numpy as np
    import torch
    from fountain_amd import default_backend
    from fountain_amd import vectorblur as V
    be = default_backend()
    img, motion, gb12 = inputs(a.res)
    h, w = img.shape[:2]
    n = w * h
    t_rgb, t_m, t_gb = (torch.from_numpy(x).cuda() for x in (img, motion, gb12))
    t_still = torch.zeros_like(t_m)
    t_out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    t_ws = torch.zeros(V.workspace_size(be, w, h) // 4, dtype=torch.float32, device="cuda")

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    if a.trace_run:
        timed(lambda: V.vector_blur_device(be, t_rgb, t_m, t_gb, t_out, t_ws))
        return
    ms = timed(lambda: t_out.copy_(t_rgb))
    copy_rate = 24 * n / statistics.median(ms) / 1e6                                # GB/s, read plus written
    out = {"image": "%dx%d" % (w, h), "field": "rotational, half velocity 0..16 pixels, clamped beyond 0.6 res from the centre", "reps": a.reps,
           "copy": {"ms": [round(x, 4) for x in ms], "median_ms": round(statistics.median(ms), 4), "GB_per_s": round(copy_rate, 1)}, "runs": {}}
    nb = V.velocities_cpu(be, motion, None)["neighbours"][..., 2]
    share = float((nb > 0.25).mean())
    out["blurred_tiles_share"] = round(share, 4)
    for call, tm, tg, p, sh in (("defaults, G-buffer", t_m, t_gb, dict(), share), ("defaults, no G-buffer", t_m, None, dict(), share),
                                ("64 taps, G-buffer", t_m, t_gb, dict(taps=64), share), ("no motion (copy)", t_still, t_gb, dict(), 0.0)):
        ms = timed(lambda: V.vector_blur_device(be, t_rgb, tm, tg, t_out, t_ws, None, p))
        nbytes = call_bytes(n, sh, tg is not None)[1]
        med = statistics.median(ms)
        out["runs"][call] = {"ms": [round(x, 4) for x in ms], "median_ms": round(med, 4), "floor_bytes": nbytes, "floor_GB_per_s": round(nbytes / med / 1e6, 1),
                             "ms_at_copy_rate": round(nbytes / copy_rate / 1e6, 4), "ratio_to_copy_rate": round(med / (nbytes / copy_rate / 1e6), 3)}
        print(call, out["runs"][call], flush=True)
        if call == "defaults, G-buffer":
            assert np.array_equal(t_out.cpu().numpy().view(np.uint32), V.vector_blur_cpu(be, img, motion, gb12).view(np.uint32)), "the device differs from the twin"
        if call == "no motion (copy)":
            assert np.array_equal(t_out.cpu().numpy().view(np.uint32), img.view(np.uint32)), "no motion must copy"
    if a.kernel_trace:
        out["per_launch_defaults"] = per_kernel(a.kernel_trace, a.reps, call_bytes(n, share, True)[0])
        for row in out["per_launch_defaults"]:
            print(row, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
