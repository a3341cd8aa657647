"""Cost of the measuring stage (ftn_metrics_device) on device buffers:
  python tools/gpu_metrics_probe.py [--res 4096] [--reps 20] [--out profiles/metrics/probe.json]
compares two seeded random images of --res squared, without and with SSIM, each without and with the maps.  Each figure is the median
of --reps calls timed with HIP events on the stream, after two warm-up calls.  Beside each stands the bytes the call must move (both
images read once, 24 bytes a pixel, and 4 bytes a pixel for each map written; the tile records are under 2 % of that) and the time they
would take at the copy rate measured in the same session (a device-to-device copy of one image, read plus written: the same number
of bytes, more than the last-level cache holds).  Before anything is timed the device's totals are checked against the host twin's at
--check-res (default 512)."""
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
    ap.add_argument("--check-res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics", "probe.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from fountain_amd import _abi as A, default_backend
    from fountain_amd import metrics as M
    be = default_backend()
    stream = torch.cuda.current_stream().cuda_stream

    def images(res):
        rng = np.random.default_rng(res)
        ref = rng.random((res, res, 3), dtype=np.float32)
        return (ref + 0.1 * rng.standard_normal((res, res, 3), dtype=np.float32)).astype(np.float32), ref

    def buffers(res, test, ref):
        t = dict(test=torch.from_numpy(test).cuda(), ref=torch.from_numpy(ref).cuda(),
                 tot=torch.zeros(A.SIZES["ftn_metrics_totals"] // 8, dtype=torch.float64, device="cuda"),
                 err=torch.zeros((res, res), dtype=torch.float32, device="cuda"), ssim=torch.zeros((res, res), dtype=torch.float32, device="cuda"),
                 ws=torch.zeros(M.workspace_size(be, res, res) // 8, dtype=torch.float64, device="cuda"))
        return t

    def call(t, res, ssim, maps):
        M.compare_device(be, t["test"].data_ptr(), t["ref"].data_ptr(), res, res, t["tot"].data_ptr(), t["ws"].data_ptr(), stream, dict(ssim=ssim),
                         error_map_ptr=t["err"].data_ptr() if maps else 0, ssim_map_ptr=t["ssim"].data_ptr() if maps and ssim else 0)

    def timed(fn):
        fn()
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

    # the device against the twin, at a size the twin does quickly
    test, ref = images(a.check_res)
    t = buffers(a.check_res, test, ref)
    for ssim in (False, True):
        call(t, a.check_res, ssim, False)
        torch.cuda.synchronize()
        got = M._struct_dict(A.ftn_metrics_totals.from_buffer_copy(t["tot"].cpu().numpy().tobytes()))
        want = M.compare_cpu(be, test, ref, dict(ssim=ssim), totals=True)["totals"]
        assert np.array_equal(np.array(got["sum"]).view(np.uint64), np.array(want["sum"]).view(np.uint64)) and {k: v for k, v in got.items() if k != "sum"} == {
            k: v for k, v in want.items() if k != "sum"}, "the device differs from the twin"
    del t

    res = a.res
    n = res * res
    test, ref = images(res)
    t = buffers(res, test, ref)
    out = {"image": "%dx%d" % (res, res), "reps": a.reps, "device": torch.cuda.get_device_name(0), "runs": {}}
    spare = torch.empty_like(t["ref"])
    ms = timed(lambda: spare.copy_(t["ref"]))                                       # 24 bytes a pixel as well: more than the last-level cache holds
    copy_rate = 24 * n / statistics.median(ms) / 1e6                                # GB/s, read plus written
    del spare
    out["runs"]["copy of one image"] = {"median_ms": round(statistics.median(ms), 4), "GB_per_s": round(copy_rate, 1)}
    for name, ssim, maps in (("pointwise", False, False), ("pointwise + error map", False, True), ("ssim", True, False), ("ssim + both maps", True, True)):
        ms = timed(lambda: call(t, res, ssim, maps))
        nbytes = 24 * n + (4 * n if maps else 0) + (4 * n if maps and ssim else 0)
        med = statistics.median(ms)
        out["runs"][name] = {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "bytes": nbytes,
                             "GB_per_s": round(nbytes / med / 1e6, 1), "ms_at_copy_rate": round(nbytes / copy_rate / 1e6, 4),
                             "ratio_to_copy_rate": round(med / (nbytes / copy_rate / 1e6), 3)}
        print(name, out["runs"][name], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
