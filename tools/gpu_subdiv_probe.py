"""Cost of Loop subdivision (include/fountain_hip_subdiv.h): the device path against the host twin, in one session on one machine:
  python tools/gpu_subdiv_probe.py [--reps 3] [--threads 16] [--out profiles/subdiv/probe.json] [--kernel-trace K.csv] [--memcpy-trace M.csv]
on bumped control grids refined five times to about 1e5, 1e6 and 1e7 faces (n x n vertices, 2 (n - 1)^2 faces, n = 8, 23, 71), and on
small ones (128 to 32 768 faces) that show where the call's fixed cost -- allocations, copies, launches -- leaves the twin ahead.  Per size:
  host_tables_ms   ftn_loop_subdivide_info: the validation and the level-0 tables, which both paths run on the host first
  device_ms        ftn_loop_subdivide, host buffers in, host buffers out: tables, allocations, uploads, kernels, downloads (a host clock;
                   the call ends in synchronous copies)
  twin_ms          ftn_loop_subdivide_cpu on --threads host threads
each the median of --reps calls after one warm-up call, and the outputs of the two compared bit for bit.  The kernels of a call run
back to back on one stream, so their times come from a trace of this very program: run it once more under
`rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -- python tools/gpu_subdiv_probe.py --trace-run`, then pass the trace's
*_kernel_trace.csv and *_memory_copy_trace.csv; the last call of the trace (the largest grid) is reported per kernel name, summed over the
levels, and per copy direction."""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GRIDS = (8, 23, 71)
LEVELS = 5
SMALL = ((2, 3), (2, 4), (2, 5), (3, 5), (5, 5))            # (n, levels): 128, 512, 2048, 8192 and 32 768 faces


def grid(n):
    import numpy as np
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    z = 0.25 * np.sin(1.3 * x + 0.2) * np.cos(0.9 * y - 0.4)
    P = np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float32)
    a = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None, :]).ravel()
    idx = np.stack([np.stack([a, a + 1, a + n + 1], 1), np.stack([a, a + n + 1, a + n], 1)], 1).reshape(-1, 3).astype(np.uint32)
    return np.ascontiguousarray(P), np.ascontiguousarray(idx)


def timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return [round(x, 3) for x in ms], round(statistics.median(ms), 3)


def last_call(kernel_csv, memcpy_csv, levels):
    """the kernels of the trace's last call by name (summed over the levels) and its copies by direction"""
    rows = [r for r in csv.DictReader(open(kernel_csv)) if "k_sd_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    n = 2 + 5 * levels + 1                                   # limit, normal, five per level, the flag words
    rows = rows[-n:]
    t0 = int(rows[0]["Start_Timestamp"])
    out = {"kernels_us": {}, "copies": {}}
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("ftn::", "")
        out["kernels_us"][name] = round(out["kernels_us"].get(name, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, 2)
    out["kernels_total_us"] = round(sum(out["kernels_us"].values()), 2)
    out["first_kernel_to_last_us"] = round((int(rows[-1]["End_Timestamp"]) - t0) / 1e3, 2)
    if memcpy_csv:
        copies = sorted(csv.DictReader(open(memcpy_csv)), key=lambda r: int(r["Start_Timestamp"]))
        t1 = int(rows[-1]["End_Timestamp"])
        up = [r for r in copies if int(r["End_Timestamp"]) <= t0][-5:]          # P, idx, nb, sf, bd of the last call
        down = [r for r in copies if int(r["Start_Timestamp"]) >= t1][:4]        # the flag words, P, N, idx
        for what, rs in (("host_to_device", up), ("device_to_host", down)):
            out["copies"][what] = {"count": len(rs), "us": round(sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rs) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subdiv", "probe.json"))
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--memcpy-trace", default=None)
    ap.add_argument("--trace-run", action="store_true", help="only a warm-up and one device call on the largest grid; writes nothing")
    a = ap.parse_args()
    import numpy as np
    from fountain_amd import _abi as A
    from fountain_amd import default_backend, subdiv
    be = default_backend()
    if be.fn("device_count")() < 1:
        raise SystemExit("gpu_subdiv_probe.py needs an AMD GPU: a time taken without one says nothing")
    lib = subdiv._lib(be)[1]
    os.environ["FTN_BVH_THREADS"] = str(a.threads)
    out = {"reps": a.reps, "twin_threads": a.threads, "sizes": []}
    for n, levels in ([(GRIDS[-1], LEVELS)] if a.trace_run else [(g, LEVELS) for g in GRIDS] + list(SMALL)):
        P, idx = grid(n)
        info = subdiv.info(be, idx, P.shape[0], levels)
        nv, nf = info.n_vertices[levels], info.n_faces[levels]
        dev = [np.empty((nv, 3), np.float32), np.empty((nv, 3), np.float32), np.empty((nf, 3), np.uint32)]
        cpu = [np.empty_like(x) for x in dev]
        head = (P.ctypes.data, P.shape[0], idx.ctypes.data, idx.shape[0], levels)
        run_dev = lambda: be.check(lib.ftn_loop_subdivide(*(head + tuple(x.ctypes.data for x in dev) + (-1,))))
        if a.trace_run:
            run_dev()
            run_dev()
            return
        scratch = A.ftn_subdiv_info()
        row = {"control": "%dx%d grid, %d faces" % (n, n, idx.shape[0]), "levels": levels, "faces": nf, "vertices": nv}
        row["host_tables_ms"], row["host_tables_median_ms"] = timed(lambda: be.check(lib.ftn_loop_subdivide_info(idx.ctypes.data, P.shape[0], idx.shape[0], levels, C.byref(scratch))), a.reps)
        row["device_ms"], row["device_median_ms"] = timed(run_dev, a.reps)
        row["twin_ms"], row["twin_median_ms"] = timed(lambda: be.check(lib.ftn_loop_subdivide_cpu(*(head + tuple(x.ctypes.data for x in cpu)))), a.reps)
        row["twin_over_device"] = round(row["twin_median_ms"] / row["device_median_ms"], 3)
        row["bytes_up"] = int(P.nbytes + 2 * idx.nbytes + 5 * P.shape[0])
        row["bytes_down"] = int(sum(x.nbytes for x in dev))
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(dev, cpu)), "the device differs from the twin"
        row["device_equals_twin"] = True
        print(row, flush=True)
        out["sizes"].append(row)
    if a.kernel_trace:
        key = "last_call_of_trace_%d_faces" % max(r["faces"] for r in out["sizes"])
        out[key] = last_call(a.kernel_trace, a.memcpy_trace, 5)
        print(out[key], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
