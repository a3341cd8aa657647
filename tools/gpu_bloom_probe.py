"""Cost of the bloom stage (ftn_bloom_device) on device buffers:
  python tools/gpu_bloom_probe.py [--res 4096] [--spp 4] [--reps 3] [--out profiles/bloom/probe.json] [--kernel-trace FILE.csv]
once on a rendered image (the Cornell box at --res squared, --spp samples) and once on a constant one.  Each figure is the median of
--reps calls timed with HIP events on the stream, after one warm-up call.  Beside each whole call stands the time its bytes would take at
the copy rate measured in the same session (a device-to-device copy of the image, read plus written): the input read twice (first
down-sampling, composite), the output written once, and every level k >= 1 written by its down-sampling, read by the next one, read and
rewritten by its blend and read by the tent above it.  A call launches its kernels back to back on one stream, so the time of each
kernel comes from a kernel trace of this very program: run it once more under `rocprofv3 --kernel-trace --output-format csv -- python
tools/gpu_bloom_probe.py --trace-run`, then pass the trace's *_kernel_trace.csv as --kernel-trace; the last --reps calls of the trace
(default parameters, rendered image) are reported per launch in launch order."""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def level_sizes(w, h, levels):
    out = []
    while len(out) < levels and (w > 1 or h > 1):
        w, h = (w + 1) >> 1, (h + 1) >> 1
        out.append((w, h))
    return out


def call_bytes(w, h, levels):
    """bytes one call must move: per launch, in launch order, and in all"""
    lv = level_sizes(w, h, levels)
    px = [w * h] + [a * b for a, b in lv]
    L = len(lv)
    launches = [("down %d->%d" % (k, k + 1), 12 * (px[k] + px[k + 1])) for k in range(L)]
    launches += [("up_blend %d" % k, 12 * (2 * px[k] + px[k + 1])) for k in range(L - 1, 0, -1)]
    launches += [("composite", 12 * (2 * px[0] + px[1]))]
    return launches, sum(b for _, b in launches)


def per_kernel(trace_csv, reps, launches):
    rows = [r for r in csv.DictReader(open(trace_csv)) if "k_bloom" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    n = len(launches)
    rows = rows[-reps * n:]
    assert len(rows) == reps * n, "the trace holds fewer bloom launches than --reps calls"
    out = []
    for i, (what, nbytes) in enumerate(launches):
        us = [(int(rows[c * n + i]["End_Timestamp"]) - int(rows[c * n + i]["Start_Timestamp"])) / 1e3 for c in range(reps)]
        name = rows[i]["Kernel_Name"].split("(")[0].replace("void ", "").replace("ftn::", "")
        med = statistics.median(us)
        out.append({"launch": what, "kernel": name, "us": [round(x, 2) for x in us], "median_us": round(med, 2), "bytes": nbytes,
                    "GB_per_s": round(nbytes / med / 1e3, 1)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=4096)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bloom", "probe.json"))
    ap.add_argument("--kernel-trace", default=None, help="the kernel trace (csv) of a --trace-run of this program")
    ap.add_argument("--trace-run", action="store_true", help="only the warm-up and --reps default calls on the rendered image; writes nothing")
    a = ap.parse_args()
    import numpy as np
    import torch
    from fountain_amd import PathIntegrator, RandomSampler, default_backend, scenes
    from fountain_amd import bloom as B
    be = default_backend()
    b, cam, res = scenes.cornell(be, res=a.res)
    rendered, _, st, _ = scenes.render(be, b, cam, res, PathIntegrator(5, 1.0), RandomSampler(a.spp, 0, indexed=True))
    rendered = np.ascontiguousarray(rendered, dtype=np.float32)
    h, w = rendered.shape[:2]
    n = w * h
    stream = torch.cuda.current_stream().cuda_stream
    t_out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    t_ws = torch.zeros(B.workspace_size(be, w, h, 12) // 4 + 4, dtype=torch.float32, device="cuda")

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
        t_rgb = torch.from_numpy(rendered).cuda()
        timed(lambda: B.bloom_device(be, t_rgb.data_ptr(), w, h, t_out.data_ptr(), t_ws.data_ptr(), stream))
        return
    out = {"image": "%dx%d" % (w, h), "rendered": "Cornell box, %d spp, PathIntegrator(5, 1.0)" % a.spp, "reps": a.reps, "runs": {}}
    for name, img in (("rendered", rendered), ("constant", np.full_like(rendered, 0.35))):
        t_rgb = torch.from_numpy(img).cuda()
        ms = timed(lambda: t_out.copy_(t_rgb))
        copy_rate = 24 * n / statistics.median(ms) / 1e6                             # GB/s, read plus written
        runs = {"copy": {"ms": [round(x, 4) for x in ms], "median_ms": round(statistics.median(ms), 4), "GB_per_s": round(copy_rate, 1)}}
        for call, p in (("default (6 levels)", dict()), ("1 level", dict(levels=1)), ("12 levels", dict(levels=12)), ("karis", dict(karis=True)),
                        ("threshold 1 knee 0.5", dict(threshold=1.0, knee=0.5)), ("exact copy (strength 0)", dict(strength=0.0))):
            ms = timed(lambda: B.bloom_device(be, t_rgb.data_ptr(), w, h, t_out.data_ptr(), t_ws.data_ptr(), stream, p))
            nbytes = 24 * n if p.get("strength") == 0.0 else call_bytes(w, h, p.get("levels", 6))[1]
            med = statistics.median(ms)
            runs[call] = {"ms": [round(x, 4) for x in ms], "median_ms": round(med, 4), "bytes": nbytes, "GB_per_s": round(nbytes / med / 1e6, 1),
                          "ms_at_copy_rate": round(nbytes / copy_rate / 1e6, 4), "ratio_to_copy_rate": round(med / (nbytes / copy_rate / 1e6), 3)}
            print(name, call, runs[call], flush=True)
            got = t_out.cpu().numpy()
            if name == "constant":
                assert np.array_equal(got.view(np.uint32), img.view(np.uint32)), "a constant image must come back unchanged"
            elif call == "default (6 levels)":
                assert np.array_equal(got.view(np.uint32), B.bloom_cpu(be, img).view(np.uint32)), "the device differs from the twin"
        out["runs"][name] = runs
        del t_rgb
    if a.kernel_trace:
        out["per_launch_default_rendered"] = per_kernel(a.kernel_trace, a.reps, call_bytes(w, h, 6)[0])
        for row in out["per_launch_default_rendered"]:
            print(row, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
