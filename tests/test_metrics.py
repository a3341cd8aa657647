"""The measuring stage on the GPU (include/fountain_hip_metrics.h, fountain_amd/metrics.py): ftn_metrics and ftn_metrics_device equal
the host twin bit for bit -- every field of the totals and the result, the tile sums, both maps with their NaN positions -- with and
without SSIM, on random and on HDR inputs, at sizes with no window, one window, one tile, clipped tiles, a total's tree that needs
padding, halos that cross tile borders, and more tiles than one workgroup of the total's reduction takes; the device entry on a torch
stream with a workspace of exactly its size between guard words; test and ref the same buffer; bad pixels; one end-to-end use: a
denoised Cornell box measures better than the noisy one; and the two command lines."""
import numpy as np
import pytest

from fountain_amd import _abi as A
from fountain_amd import metrics as M

import _metrics_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SIZES = [(1, 1), (5, 33), (11, 11), (12, 11), (16, 16), (17, 16), (16, 17), (48, 16), (80, 16), (27, 43), (272, 272)]       # (w, h)
ALL = dict(error_map=True, tile_sums=True, totals=True)
bits32, bits64 = R.bits32, R.bits64


def assert_same(got, want, ssim, what):
    """every field, bit for bit (NaN fields compare as bit patterns too)"""
    for k in M.RESULT_FIELDS:
        assert np.array_equal(bits64(got[k]), bits64(want[k])) if isinstance(want[k], (float, tuple)) else got[k] == want[k], (what, k, got[k], want[k])
    for k, v in want["totals"].items():
        assert np.array_equal(bits64(got["totals"][k]), bits64(v)) if isinstance(v, (float, tuple)) else got["totals"][k] == v, (what, k, got["totals"][k], v)
    assert np.array_equal(bits64(got["tile_sums"]), bits64(want["tile_sums"])), (what, "tile_sums")
    assert np.array_equal(bits32(got["error_map"]), bits32(want["error_map"])), (what, "error_map")
    if ssim:
        assert np.array_equal(bits32(got["ssim_map"]), bits32(want["ssim_map"])), (what, "ssim_map")


def run_device(gpu, test, ref, params, ssim, same=False, stream=None):
    """ftn_metrics_device over torch tensors on `stream` (None: a new one); the workspace is exactly workspace_size bytes between two
    guard words.  Returns compare()'s dict."""
    import torch
    h, w = test.shape[:2]
    nbytes = M.workspace_size(gpu, w, h, params.desc.flags)
    assert nbytes % 16 == 0
    guard = 0x5ca1ab1e
    s = stream or torch.cuda.Stream()
    with torch.cuda.stream(s):
        t_test = torch.from_numpy(test).cuda()
        t_ref = t_test if same else torch.from_numpy(ref).cuda()
        t_tot = torch.full((A.SIZES["ftn_metrics_totals"] // 4,), -1, dtype=torch.int32, device="cuda")
        t_err = torch.full((h, w), 7.0, dtype=torch.float32, device="cuda")
        t_ssim = torch.full((h, w), 7.0, dtype=torch.float32, device="cuda")
        t_tiles = torch.full((M.n_tiles(w, h), 8), 7.0, dtype=torch.float64, device="cuda")
        t_ws = torch.full((nbytes // 4 + 8,), guard, dtype=torch.int32, device="cuda")            # 16 bytes of guard on either side
        M.compare_device(gpu, t_test.data_ptr(), t_ref.data_ptr(), w, h, t_tot.data_ptr(), t_ws.data_ptr() + 16, s.cuda_stream, params,
                         error_map_ptr=t_err.data_ptr(), ssim_map_ptr=t_ssim.data_ptr() if ssim else 0, tile_sums_ptr=t_tiles.data_ptr())
    s.synchronize()
    ws = t_ws.cpu().numpy()
    assert (ws[:4] == guard).all() and (ws[-4:] == guard).all(), "the workspace's guard words were written"
    assert np.array_equal(bits32(t_test.cpu().numpy()), bits32(test))
    tot = A.ftn_metrics_totals.from_buffer_copy(t_tot.cpu().numpy().tobytes())
    out = M.resolve(gpu, tot, params)
    out.update(totals=M._struct_dict(tot), error_map=t_err.cpu().numpy(), tile_sums=t_tiles.cpu().numpy())
    if ssim:
        out["ssim_map"] = t_ssim.cpu().numpy()
    else:
        assert (t_ssim == 7.0).all()
    return out


@pytest.mark.parametrize("scale", [1.0, 100.0], ids=["unit", "hdr"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_device_equals_twin(gpu, size, scale):
    w, h = size
    test, ref = R.images(w, h, scale=scale)
    before = test.copy(), ref.copy()
    for ssim in (False, True) if min(w, h) >= 11 else (False,):
        p = M.MetricsParams(gpu, ssim=ssim, peak=scale)
        want = M.compare_cpu(gpu, test, ref, p, ssim_map=ssim, **ALL)
        assert_same(M.compare(gpu, test, ref, p, ssim_map=ssim, **ALL), want, ssim, (size, ssim, "ftn_metrics"))
        assert_same(run_device(gpu, test, ref, p, ssim), want, ssim, (size, ssim, "ftn_metrics_device"))
    assert np.array_equal(bits32(test), bits32(before[0])) and np.array_equal(bits32(ref), bits32(before[1]))


def test_without_the_optional_outputs(gpu):
    test, ref = R.images(27, 43)
    for ssim in (False, True):
        want = M.compare_cpu(gpu, test, ref, dict(ssim=ssim))
        got = M.compare(gpu, test, ref, dict(ssim=ssim))
        assert sorted(got) == sorted(M.RESULT_FIELDS)
        for k in M.RESULT_FIELDS:
            assert np.array_equal(bits64(got[k]), bits64(want[k])), k


def test_the_same_buffer_on_both_sides(gpu):
    x, _ = R.images(43, 27, scale=100.0)
    p = M.MetricsParams(gpu, ssim=True, peak=100.0)
    want = M.compare_cpu(gpu, x, x, p, ssim_map=True, **ALL)
    assert want["ssim"] == 1.0 and want["psnr"] == float("inf") and want["n_different"] == 0
    assert_same(M.compare(gpu, x, x, p, ssim_map=True, **ALL), want, True, "ftn_metrics, test is ref")
    assert_same(run_device(gpu, x, x, p, True, same=True), want, True, "ftn_metrics_device, test is ref")


def test_bad_pixels(gpu):
    """non-finite values in a tile's corner, on a tile border, in the last row and column, the same NaN on both sides, and a whole
    tile of them; signed zeros and the largest finite values beside them"""
    w, h = 50, 37
    test, ref = R.images(w, h)
    test[0, 0, 0] = np.nan
    ref[15, 16, 1] = np.inf
    test[16, 15, 2] = -np.inf
    ref[h - 1, w - 1, 0] = np.nan
    test[20, 30] = ref[20, 30] = np.array([0x7fc12345, 0x3f800000, 0x3f800000], np.uint32).view(F32)
    test[3, 40] = (0.0, -0.0, 3.4028235e38)
    ref[3, 40] = (-0.0, -0.0, -3.4028235e38)
    for ssim in (False, True):
        p = M.MetricsParams(gpu, ssim=ssim)
        want = M.compare_cpu(gpu, test, ref, p, ssim_map=ssim, **ALL)
        assert want["n_nonfinite"] == 5 and want["max_abs_index"] == 3 * w + 40
        assert_same(M.compare(gpu, test, ref, p, ssim_map=ssim, **ALL), want, ssim, ("bad pixels", ssim, "ftn_metrics"))
        assert_same(run_device(gpu, test, ref, p, ssim), want, ssim, ("bad pixels", ssim, "ftn_metrics_device"))
    test[16:32, 16:32] = np.nan                                          # tile 5 of 12 holds no good pixel
    p = M.MetricsParams(gpu, ssim=True)
    want = M.compare_cpu(gpu, test, ref, p, ssim_map=True, **ALL)
    assert not want["tile_sums"][5].any() and want["tile_sums"][4].all()
    assert_same(M.compare(gpu, test, ref, p, ssim_map=True, **ALL), want, True, "a tile of NaN")
    none = np.full((12, 12, 3), np.nan, F32)
    want = M.compare_cpu(gpu, none, ref[:12, :12], p, ssim_map=True, **ALL)
    assert want["n"] == 0 and np.isnan(want["mse"])
    assert_same(M.compare(gpu, none, ref[:12, :12], p, ssim_map=True, **ALL), want, True, "every pixel bad")


def test_device_entry_on_the_current_stream_twice(gpu):
    """two calls in a row on one stream into the same workspace: nothing is carried over from the first"""
    import torch
    s = torch.cuda.Stream()
    p = M.MetricsParams(gpu, ssim=True)
    for seed in (3, 4):
        test, ref = R.images(272, 33, seed=seed)
        assert_same(run_device(gpu, test, ref, p, True, stream=s), M.compare_cpu(gpu, test, ref, p, ssim_map=True, **ALL), True, seed)


def test_denoised_cornell_measures_better(gpu):
    """Cornell at 64 x 64: a 4-spp render and its variance-guided denoising against a 256-spp render of the same scene"""
    from fountain_amd import PathIntegrator, RandomSampler, denoise as D, gbuffer as G, moments as MO, scenes
    b, cam, res = scenes.cornell(gpu, res=64)
    scene = b.create_scene()
    ref, _, _, _ = scenes.render(gpu, b, cam, res, PathIntegrator(5, 1.0), RandomSampler(256, 77, indexed=True))
    smp = RandomSampler(4, 5, indexed=True)
    var4, film, _, _ = MO.render_moments(gpu, None, cam, res, PathIntegrator(5, 1.0), smp, scene=scene)
    noisy, _ = film.into_spectrum_buffer()
    r, _, _ = G.render_gbuffer(gpu, None, cam, res, smp, scene=scene)
    denoised = D.denoise_guided(gpu, noisy, np.concatenate([r[k] for k in G.CHANNELS], axis=-1), var4)
    ref = np.ascontiguousarray(ref, F32)
    n, d = M.compare(gpu, noisy, ref, dict(ssim=True)), M.compare(gpu, denoised, ref, dict(ssim=True))
    print("Cornell 64^2 against 256 spp: 4 spp rel_mse %.5g ssim %.5g; denoised rel_mse %.5g ssim %.5g" % (n["rel_mse"], n["ssim"], d["rel_mse"], d["ssim"]))
    assert d["rel_mse"] < n["rel_mse"] and d["ssim"] > n["ssim"]


def test_command_lines(gpu, tmp_path, capsys):
    """render.py --compare-to prints the line of fountain_amd.metrics for the image just written and writes what it writes without the
    option; the metrics command line on the GPU prints what --cpu prints"""
    import os
    from fountain_amd import render
    scene_file = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "cornell.pbrt")
    ref, plain, out = str(tmp_path / "ref.exr"), tmp_path / "plain", tmp_path / "out"
    plain.mkdir()
    out.mkdir()
    assert render.main([scene_file, "-o", ref, "--samples", "16"]) == 0
    assert render.main([scene_file, "-o", str(plain / "a.exr"), "--samples", "4"]) == 0
    capsys.readouterr()
    assert render.main([scene_file, "-o", str(out / "a.exr"), "--samples", "4", "--compare-to", ref, "--ssim"]) == 0
    line = capsys.readouterr().out
    assert sorted(f.name for f in out.iterdir()) == ["a.exr"] and (out / "a.exr").read_bytes() == (plain / "a.exr").read_bytes()
    assert M.main([str(out / "a.exr"), ref, "--ssim"]) == 0
    assert capsys.readouterr().out == line and line.startswith("metrics: rmse ") and " ssim 0." in line and "4096 pixels differ" in line
    assert M.main([str(out / "a.exr"), ref, "--ssim", "--cpu"]) == 0
    assert capsys.readouterr().out == line
    # an image against itself, through the files
    capsys.readouterr()
    assert render.main([scene_file, "-o", str(out / "b.exr"), "--samples", "16", "--compare-to", ref]) == 0
    assert "0 of 4096 pixels differ" in capsys.readouterr().out and M.main([str(out / "b.exr"), ref, "--fail-above", "n_different=0", "--fail-above", "rmse=0"]) == 0
    assert M.main([str(out / "a.exr"), ref, "--fail-above", "rmse=1e-4"]) == 1
