"""bench.py's one JSON line: the fields the driver's contract names are present, typed and mutually consistent -- checked on the line of
the last profiled run (profiles/r03/bench.json, the line of what is now `python bench.py --full --steps 10 --warmup 2`: a plain run leaves the
roofline and cpu_baseline blocks out) and on the helper
functions the line is built from.  CPU only; the line itself is produced on a GPU (tests/test_multigpu_gloo.py runs bench.py end to end
there)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_line():
    path = os.path.join(ROOT, "profiles", "r03", "bench.json")
    lines = [l for l in open(path).read().splitlines() if l.startswith("{")]
    assert len(lines) == 1, "stdout of bench.py carries the result line alone"
    return json.loads(lines[0])


def test_contract_fields():
    b = load_line()
    for k, t in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int), ("ms_per_step", float),
                 ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str), ("config", dict), ("roofline", dict), ("cpu_baseline", dict)):
        assert isinstance(b[k], t), k
    assert b["vs_baseline"] is None                     # BASELINE.md holds no published number for this metric
    assert b["unit"] == "Mrays/s" and b["higher_is_better"] is True and b["scaling"] in ("weak", "strong") and b["dtype"] == "f32" and b["data"] == "synthetic"
    assert "workload" in b["config"] and "model" not in b["config"] and "10002588 triangles" in b["config"]["workload"]
    # value = rays of all ranks / wall time of the timed steps
    assert abs(b["config"]["rays_per_step"] / (b["ms_per_step"] * 1e-3) / 1e6 - b["value"]) / b["value"] < 1e-3
    assert b["config"]["device_ms_per_step"] <= b["ms_per_step"] * 1.001
    # (2.98 GB of scene arrays + 134 MB of environment cell records)
    assert sum(v for k, v in b["config"]["device_bytes"].items() if k != "total_bytes") == b["config"]["device_bytes"]["total_bytes"] < 3.2e9
    assert b["config"]["device_bytes"]["total_bytes"] - b["config"]["device_bytes"]["lights_bytes"] < 3.0e9
    for k in ("device_ms_per_step", "render_wall_ms", "merge_ms"):
        assert 0 <= b["ranks"][k]["min"] <= b["ranks"][k]["max"]


def test_roofline_block():
    r = load_line()["roofline"]
    assert r["unit"] == "GB/s" and r["peak"] == 8000.0 and 0 < r["frac"] <= 1.0
    assert abs(r["achieved"] / r["peak"] - r["frac"]) < 1e-3
    assert abs(r["traffic"] / (r["avg_launch_ms"] * 1e-3) / 1e9 - r["achieved"]) / r["achieved"] < 1e-3          # counter bytes per launch / live launch time
    assert r["bound"] in ("memory_latency", "valu_issue", "hbm")
    i = r["issue"]
    assert abs(i["valu_busy"] * i["lanes_per_valu_inst"] / i["of_lanes"] - i["frac"]) < 1e-3 and 0 < i["frac"] <= 1.0
    assert r["hbm"]["frac"] == r["frac"] and r["hbm"]["traffic"] == r["traffic"]
    g = r["groups"]
    assert set(g) >= {"closest", "any_hit", "shade", "other"} and all(v["ms_per_step"] is not None and v["ms_per_step"] >= 0 for v in g.values())
    assert abs(sum(v["ms_per_step"] for v in g.values()) - r["whole_step"]["device_ms"]) < 0.05 * r["whole_step"]["device_ms"]
    assert 0 < r["whole_step"]["hbm_frac"] <= 1.0 and g["shade"]["hbm_bytes_per_event"] > 0
    # algorithmic bytes are reported, but never as a fraction of the HBM roof
    assert "GB_per_s" in r["algorithmic"] and "frac" not in r["algorithmic"]


def test_cpu_baseline_block():
    c = load_line()["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "Mrays/s" and c["cores"] >= 1 and c["value"] > 0 and "tiles" in c["sample"]


def test_step_and_workload_helpers():
    import argparse
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    a = argparse.Namespace(copies=2309, res=4096, spp_per_gpu=16, scaling="weak", gpus=8)
    assert bench.per_gpu_workload(a) == "copies=2309,res=4096,spp_per_gpu=16"      # weak: one GPU's share does not depend on N
    a.scaling = "strong"
    assert bench.per_gpu_workload(a) == "copies=2309,res=4096,spp=16,tiles=1/8"
    a.gpus = 1
    assert bench.per_gpu_workload(a) == "copies=2309,res=4096,spp_per_gpu=16"
    assert bench.PROFILE_ROUND == "r03" and os.path.exists(os.path.join(ROOT, "profiles", bench.PROFILE_ROUND, "traffic.json"))
    tj = json.load(open(os.path.join(ROOT, "profiles", bench.PROFILE_ROUND, "traffic.json")))
    if tj["source_hash"] != bench.source_hash():          # (bench.py then leaves the HBM-side figures out of its line and says so: no silent staleness)
        pytest.skip("profiles/r03/traffic.json was taken on other kernel sources: rerun tools/make_traffic_json.py on the GPU box")


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs(tmp_path):
    """--dump-outputs: a small film is written whole, a large one as the same fixed sample on every run; float32 / float64 only,
    64 MB at most for the benchmark's 4096 x 4096 film."""
    import numpy as np
    import torch
    bench = _load_bench()
    st = {k: 1000 + i for i, k in enumerate(bench.LAST_STEP_COUNTERS)}
    small = torch.arange(8 * 6 * 4, dtype=torch.float32).reshape(8, 6, 4)
    bench.dump_outputs(str(tmp_path / "small"), small, st)
    px = np.load(tmp_path / "small" / "film_pixels.npy")
    assert px.dtype == np.float32 and np.array_equal(px, small.numpy().reshape(-1, 4))
    assert np.array_equal(np.load(tmp_path / "small" / "film_pixel_index.npy"), np.arange(48, dtype=np.float64))
    c = np.load(tmp_path / "small" / "last_step_counts.npy")
    assert c.dtype == np.float64 and list(c) == [float(st[k]) for k in bench.LAST_STEP_COUNTERS]

    big = torch.rand((4096, 4096, 4), generator=torch.Generator().manual_seed(1))
    runs = []
    for name in ("a", "b"):
        d = tmp_path / name
        bench.dump_outputs(str(d), big, None)
        files = sorted(d.iterdir())
        assert [f.name for f in files] == ["film_pixel_index.npy", "film_pixels.npy", "last_step_counts.npy"]
        assert sum(f.stat().st_size for f in files) <= 64 << 20
        arrs = {f.stem: np.load(f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
        runs.append(arrs)
    idx = runs[0]["film_pixel_index"]
    assert len(idx) == bench.DUMP_MAX_PIXELS and np.all(np.diff(idx) > 0) and idx[-1] < 4096 * 4096
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
    assert np.array_equal(runs[0]["film_pixels"], big.numpy().reshape(-1, 4)[idx.astype(np.int64)])
    assert not runs[0]["last_step_counts"].any()


SMALL = ["--gpus", "1", "--copies", "8", "--res", "256", "--spp-per-gpu", "2", "--steps", "2", "--warmup", "1"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout                      # stdout carries the result line alone
    return json.loads(lines[0])


def test_full_is_an_option_of_every_run():
    """--full is off by default and parses beside the other options (no GPU: --launch-check stops before any rendering)"""
    env = dict(os.environ, OMP_NUM_THREADS="1", HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    for extra in ([], ["--full"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--launch-check"] + extra, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        assert json.loads(r.stdout.strip().splitlines()[-1])["n_gpus"] == 1


@pytest.mark.gpu
def test_plain_run_is_lean_and_full_run_adds_the_rest(tmp_path):
    """a plain run prints the headline fields without the blocks that take runs of their own; --full adds the roofline block (with the
    counting step's `algorithmic` part) and the CPU baseline, and changes neither the meaning of the headline fields nor one bit of
    what --dump-outputs writes"""
    import numpy as np
    plain = _bench(SMALL + ["--dump-outputs", str(tmp_path / "plain")])
    full = _bench(SMALL + ["--full", "--dump-outputs", str(tmp_path / "full")])
    for out in (plain, full):
        assert all(k in out for k in HEADLINE) and out["value"] > 0 and out["ms_per_step"] > 0
        assert abs(out["config"]["rays_per_step"] / (out["ms_per_step"] * 1e-3) / 1e6 - out["value"]) / out["value"] < 1e-2
    assert "roofline" not in plain and "cpu_baseline" not in plain
    assert "algorithmic" in full["roofline"] and full["roofline"]["launches_per_step"] > 0
    assert full["cpu_baseline"]["kind"] == "port" and full["cpu_baseline"]["value"] > 0
    for k in HEADLINE:
        if k not in ("value", "ms_per_step"):
            assert plain[k] == full[k], k
    assert plain["config"]["rays_per_step"] == full["config"]["rays_per_step"]
    for name in ("film_pixels.npy", "film_pixel_index.npy", "last_step_counts.npy"):
        a, b = np.load(tmp_path / "plain" / name), np.load(tmp_path / "full" / name)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
