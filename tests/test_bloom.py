"""The bloom stage on the GPU (include/fountain_hip_bloom.h, fountain_amd/bloom.py): the device equals the host twin bit for bit on
images of one pixel, one row, one column, less than a tile, tiles with ragged edges and several workgroups, at every depth, with both
flags and thresholds, and on the salted image; the exact copies; the device entry on a torch stream into sentinel-filled buffers and in
a captured graph; a rendered Cornell box; inputs untouched and repeated calls; the three command lines.  No kernel caps its grid (one
workgroup per tile or per 1024 pixels), so no size beyond 255 x 257 is needed."""
import itertools
import os

import numpy as np
import pytest

from fountain_amd import bloom as B
from fountain_amd import display as D

import _bloom_common as K
import _display_ref as DR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
bits = K.bits
CASES = [dict(levels=lv, karis=karis, strength=0.5, **th) for lv, karis, th in
         itertools.product(K.LEVELS, (False, True), (dict(threshold=0.0), dict(threshold=1.0, knee=0.5)))]


@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: "%dx%d" % s)
def test_device_equals_twin(gpu, size):
    img = K.image(*size)
    before = img.copy()
    for p in CASES:
        got, want = B.bloom(gpu, img, p), B.bloom_cpu(gpu, img, p)
        assert np.array_equal(bits(got), bits(want)), (size, p, int((bits(got) != bits(want)).sum()))
    for p in (dict(), dict(scatter=0.0, strength=1.0), dict(scatter=1.0, strength=1.0, levels=3), dict(clamp_max=0.5, threshold=0.25, knee=1.0)):
        assert np.array_equal(bits(B.bloom(gpu, img, p)), bits(B.bloom_cpu(gpu, img, p))), (size, p)
    assert np.array_equal(bits(img), bits(before))


def test_salted_image_and_exact_copies(gpu):
    img, _ = K.salted()
    img[5, 6] = np.array([0x7fc12345, 0xffc00001, 0x7f800001], np.uint32).view(F32)          # NaNs with payloads
    for p in CASES[:4] + CASES[-4:]:
        got, want = B.bloom(gpu, img, p), B.bloom_cpu(gpu, img, p)
        assert np.array_equal(bits(got), bits(want)), p
    with np.errstate(invalid="ignore"):
        stays = ~np.isfinite(img) | (img < 0)
    assert np.array_equal(bits(B.bloom(gpu, img, dict(strength=1.0)))[stays], bits(img)[stays])
    for p in (dict(strength=0.0), dict(levels=0), dict(levels=0, strength=1.0, karis=True)):
        assert np.array_equal(bits(B.bloom(gpu, img, p)), bits(img)), p
    for shape in ((1, 1, 3), (1, 2, 3), (3, 3, 3)):                                 # 3, 6 and 27 words: the copy's tail alone, and with a group
        small = np.array([0x80000000, 0x7fc12345, 0x3f800000] * (shape[0] * shape[1]), np.uint32).view(F32).reshape(shape)
        assert np.array_equal(bits(B.bloom(gpu, small, dict(strength=0.0))), bits(small)), shape
    assert np.array_equal(bits(B.bloom(gpu, small[:1, :1], dict(strength=1.0))), bits(small[:1, :1]))


def test_constants_and_repeated_calls(gpu):
    for c in (0.0, 0.75, 3.0, 1024.0):
        img = np.full((53, 37, 3), c, F32)
        assert np.array_equal(bits(B.bloom(gpu, img)), bits(img)), c
    img = K.image(255, 257)
    first = B.bloom(gpu, img, dict(karis=True))
    assert np.array_equal(bits(B.bloom(gpu, img, dict(karis=True))), bits(first))


def test_device_entry_on_a_torch_stream(gpu):
    """ftn_bloom_device on a non-default stream, the output and the workspace pre-filled with sentinels (NaN: a read of either before
    it is written would spread)"""
    import torch
    for (w, h), p in (((5, 7), dict(strength=0.5)), ((255, 257), dict(strength=0.5, karis=True, threshold=1.0)), ((37, 53), dict(levels=12, strength=1.0)),
                      ((17, 31), dict(strength=0.0)), ((1, 1), dict()), ((5, 7), dict(levels=0, strength=1.0))):
        img = K.salted(w, h)[0] if (w, h) == (37, 53) else K.image(w, h)
        want = B.bloom_cpu(gpu, img, p)
        nbytes = B.workspace_size(gpu, w, h, p.get("levels"))
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            t_rgb = torch.from_numpy(img).cuda()
            t_out = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
            t_ws = torch.full((nbytes // 4 + 4,), float("nan"), dtype=torch.float32, device="cuda")
            # no level, no workspace: a null one is in order, and the exact copy runs over device memory
            B.bloom_device(gpu, t_rgb.data_ptr(), w, h, t_out.data_ptr(), t_ws.data_ptr() if nbytes else 0, s.cuda_stream, p)
        s.synchronize()
        assert np.array_equal(bits(t_out.cpu().numpy()), bits(want)), (w, h, p)
        assert np.array_equal(bits(t_rgb.cpu().numpy()), bits(img))
        assert torch.isnan(t_ws[nbytes // 4:]).all()                              # nothing written past the workspace's size


def test_graph_capture(gpu):
    """ftn_bloom_device captured once in a torch.cuda.graph (every buffer allocated before the capture), replayed twice with new inputs
    copied into the captured buffer; the exact copy is a kernel too and is captured likewise"""
    import torch
    w, h = 255, 257
    img = K.image(w, h)
    inputs = [K.image(w, h, seed=9), K.image(w, h, seed=10)]                    # neither is the image of the warm-up and the capture
    for p in (dict(strength=0.5, karis=True), dict(strength=0.0)):
        t_rgb = torch.from_numpy(img).cuda()
        t_out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        t_ws = torch.zeros(B.workspace_size(gpu, w, h) // 4 + 4, dtype=torch.float32, device="cuda")
        run = lambda: B.bloom_device(gpu, t_rgb.data_ptr(), w, h, t_out.data_ptr(), t_ws.data_ptr(), torch.cuda.current_stream().cuda_stream, p)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            run()                                                            # warm-up before the capture
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            run()
        for r in inputs:
            t_rgb.copy_(torch.from_numpy(r))
            t_out.fill_(float("nan"))
            t_ws.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(bits(t_out.cpu().numpy()), bits(B.bloom_cpu(gpu, r, p))), p


@pytest.fixture(scope="module")
def cornell(gpu):
    from fountain_amd import PathIntegrator, RandomSampler, scenes
    b, cam, res = scenes.cornell(gpu, res=32)
    rgb, _, _, _ = scenes.render(gpu, b, cam, res, PathIntegrator(5, 1.0), RandomSampler(4, 0, indexed=True))
    return np.ascontiguousarray(rgb, dtype=F32)


def test_rendered_cornell_box(gpu, cornell):
    before = cornell.copy()
    for p in (dict(), dict(strength=0.3, karis=True), dict(strength=0.3, threshold=0.5)):
        got = B.bloom(gpu, cornell, p)
        assert np.array_equal(bits(got), bits(B.bloom_cpu(gpu, cornell, p))), p
        assert np.isfinite(got).all() and not np.array_equal(bits(got), bits(cornell))
    assert np.array_equal(bits(cornell), bits(before))


def test_cli(gpu, tmp_path):
    """--png --bloom writes out_bloom.exr (the twin's bits of out.exr) and an out.png that is the bloomed image's, automatic exposure
    included; out.exr is byte for byte that of a run without --bloom, whose out.png is the unbloomed image's as before;
    fountain_amd.display --bloom and fountain_amd.bloom make the same pictures from the written file"""
    from fountain_amd import render
    from fountain_amd.api import read_exr
    scene_file = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")
    plain, out = tmp_path / "plain", tmp_path / "bloom"
    plain.mkdir()
    out.mkdir()
    opts = ["--bloom", "0.3", "--bloom-levels", "4", "--bloom-scatter", "0.6", "--bloom-threshold", "0.5", "--bloom-knee", "0.25", "--bloom-karis"]
    p = dict(strength=0.3, levels=4, scatter=0.6, threshold=0.5, knee=0.25, karis=True)
    assert render.main([scene_file, "-o", str(plain / "out.exr"), "--samples", "4", "--png", "--auto-exposure"]) == 0
    assert render.main([scene_file, "-o", str(out / "out.exr"), "--samples", "4", "--png", "--auto-exposure"] + opts) == 0
    assert sorted(f.name for f in plain.iterdir()) == ["out.exr", "out.png"]
    assert sorted(f.name for f in out.iterdir()) == ["out.exr", "out.png", "out_bloom.exr"]
    assert (plain / "out.exr").read_bytes() == (out / "out.exr").read_bytes()
    main = read_exr(str(out / "out.exr"), gpu)
    bloomed = B.bloom_cpu(gpu, main, p)
    assert np.array_equal(bits(read_exr(str(out / "out_bloom.exr"), gpu)), bits(bloomed))
    for directory, img in ((plain, main), (out, bloomed)):
        scale = D.exposure(gpu, D.histogram_cpu(gpu, img), dict(auto_exposure=True))["scale"]
        want, _ = DR.unpack(D.encode_cpu(gpu, img, scale))
        assert np.array_equal(DR.read_png(str(directory / "out.png"))["pixels"].astype(np.int64), want), directory.name
    assert not np.array_equal(DR.read_png(str(plain / "out.png"))["pixels"], DR.read_png(str(out / "out.png"))["pixels"])
    # the display module: without the options the picture of before, with them the bloomed one
    assert D.main([str(out / "out.exr"), "-o", str(tmp_path / "a.png"), "--auto-exposure"]) == 0
    assert np.array_equal(DR.read_png(str(tmp_path / "a.png"))["pixels"], DR.read_png(str(plain / "out.png"))["pixels"])
    assert D.main([str(out / "out.exr"), "-o", str(tmp_path / "b.png"), "--auto-exposure"] + opts) == 0
    assert np.array_equal(DR.read_png(str(tmp_path / "b.png"))["pixels"], DR.read_png(str(out / "out.png"))["pixels"])
    # the bloom module
    assert B.main([str(out / "out.exr"), "-o", str(tmp_path / "c.exr"), "--strength", "0.3", "--levels", "4", "--scatter", "0.6", "--threshold", "0.5",
                   "--knee", "0.25", "--karis"]) == 0
    assert np.array_equal(bits(read_exr(str(tmp_path / "c.exr"), gpu)), bits(bloomed))
    assert B.main([str(out / "out.exr")]) == 0                                    # the default name and parameters
    assert np.array_equal(bits(read_exr(str(out / "out_bloom.exr"), gpu)), bits(B.bloom_cpu(gpu, main)))
