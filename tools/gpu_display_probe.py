"""Cost of the display stage's two kernels (ftn_display_histogram_device, ftn_display_encode_device) on device buffers:
  python tools/gpu_display_probe.py [--res 4096] [--spp 4] [--reps 3] [--out profiles/display/probe.json]
once on a rendered image (the Cornell box at --res squared, --spp samples) and once on a constant one, the histogram's worst case:
every pixel of every lane falls into one bin.  Each figure is the median of --reps launches timed with HIP events on the stream, after
one warm-up launch; the bytes are those the kernel must move (12 per pixel read, 4 written, 12 more with the float image)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=4096)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "display", "probe.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from fountain_amd import PathIntegrator, RandomSampler, default_backend, scenes, _abi as A
    from fountain_amd import display as D
    be = default_backend()
    b, cam, res = scenes.cornell(be, res=a.res)
    rendered, _, st, _ = scenes.render(be, b, cam, res, PathIntegrator(5, 1.0), RandomSampler(a.spp, 0, indexed=True))
    rendered = np.ascontiguousarray(rendered, dtype=np.float32)
    h, w = rendered.shape[:2]
    n = w * h
    out = {"image": "%dx%d" % (w, h), "rendered": "Cornell box, %d spp, PathIntegrator(5, 1.0)" % a.spp, "reps": a.reps,
           "bytes": {"histogram": 12 * n, "encode": 16 * n, "encode_with_float_image": 28 * n}, "runs": {}}
    stream = torch.cuda.current_stream().cuda_stream
    t_hist = torch.zeros(A.FTN_DISPLAY_HIST_WORDS, dtype=torch.int32, device="cuda")
    t_8 = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    t_f = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")

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

    for name, img in (("rendered", rendered), ("constant", np.full_like(rendered, 0.35))):
        t_rgb = torch.from_numpy(img).cuda()
        hist = D.histogram_cpu(be, img)
        info = D.exposure(be, hist, dict(auto_exposure=True))
        runs = {"bins_in_use": int(np.count_nonzero(hist[:A.FTN_DISPLAY_HIST_BINS])), "largest_bin_share": float(hist.max()) / n, "scale": info["scale"]}
        calls = (("histogram", 12 * n, lambda: D.histogram_device(be, t_rgb.data_ptr(), w, h, t_hist.data_ptr(), stream)),
                 ("encode", 16 * n, lambda: D.encode_device(be, t_rgb.data_ptr(), w, h, info["scale"], None, t_8.data_ptr(), stream)),
                 ("encode_dither_hable", 16 * n, lambda: D.encode_device(be, t_rgb.data_ptr(), w, h, info["scale"], None, t_8.data_ptr(), stream,
                                                                         dict(tonemap="hable", dither=True))),
                 ("encode_with_float_image", 28 * n, lambda: D.encode_device(be, t_rgb.data_ptr(), w, h, info["scale"], t_f.data_ptr(), t_8.data_ptr(), stream)))
        for call, nbytes, fn in calls:
            ms = timed(fn)
            med = statistics.median(ms)
            runs[call] = {"ms": [round(x, 4) for x in ms], "median_ms": round(med, 4), "GB_per_s": round(nbytes / med / 1e6, 1)}
            print(name, call, runs[call], flush=True)
        assert np.array_equal(t_hist.cpu().numpy().view(np.uint32), hist), "the device histogram differs from the twin's"
        out["runs"][name] = runs
        del t_rgb
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
