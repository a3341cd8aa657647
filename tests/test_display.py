"""The display stage on the GPU (include/fountain_hip_display.h, fountain_amd/display.py): the device histogram and the device encode
equal the host twins bit for bit (codes and float image) on images that are all tail, on four-pixel groups that straddle rows, on
several workgroups, on the constant image (one bin, more than 65535 pixels), on the salted image and on an image that takes both
grid-stride loops round more than once; every curve x transfer with and without dither; both device entries on a torch stream and
in a captured graph; the whole chain on a rendered Cornell box; inputs untouched and repeated calls; the CLI."""
import os

import numpy as np
import pytest

from fountain_amd import _abi as A
from fountain_amd import display as D

import _display_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)

# both kernels run 256-thread workgroups whose threads take four pixels per trip; the encode grid is capped at 2048 workgroups and the
# histogram's at 1024 (FTN_DISPLAY_ENCODE_MAX_BLOCKS, FTN_DISPLAY_HIST_MAX_BLOCKS in ftn_display.h), fixed numbers that do not scale
# with the device.  The smallest image that sends both loops round again has more than 2048 * 256 * 4 = 2 097 152 pixels: 2049 x 1025
# = 2 100 225, odd in both directions, with a tail of one pixel.
ENCODE_CAP_PIXELS = 2048 * 256 * 4
BIG_W, BIG_H = 2049, 1025


@pytest.fixture(scope="module")
def imgs():
    out = R.images()
    assert BIG_W * BIG_H > ENCODE_CAP_PIXELS and (BIG_W * BIG_H) % 4 == 1
    out["above the grid caps"] = R.log_uniform(np.random.default_rng(8), (BIG_H, BIG_W, 3), -14.0, 8.0)
    return out


NAMES = ["random 1x1", "random 1x3", "random 3x1", "random 5x7", "random 37x53", "random 257x255", "constant 512x512", "checker 48x64",
         "salted 37x53", "above the grid caps"]


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_twin(gpu, imgs, name):
    img = imgs[name]
    before = img.copy()
    hist = D.histogram(gpu, img)
    assert np.array_equal(hist, D.histogram_cpu(gpu, img)) and int(hist.sum()) == img.shape[0] * img.shape[1]
    for p, scale in ((dict(dither=True), 0.37), (dict(tonemap="reinhard", transfer="gamma"), 1.0)):
        got8, gotf = D.encode(gpu, img, scale, p, want_float=True)
        want8, wantf = D.encode_cpu(gpu, img, scale, p, want_float=True)
        assert np.array_equal(got8, want8), (name, p, int((got8 != want8).sum()))
        assert np.array_equal(bits(gotf), bits(wantf)), (name, p)
        assert np.array_equal(D.encode(gpu, img, scale, p), want8)                         # without the float image
    assert np.array_equal(bits(img), bits(before))
    if name == "constant 512x512":
        assert hist.max() == 262144


@pytest.mark.parametrize("dither", [False, True])
@pytest.mark.parametrize("tf", R.TRANSFERS)
@pytest.mark.parametrize("tm", R.TONEMAPS)
def test_every_curve_and_transfer(gpu, imgs, tm, tf, dither):
    img = imgs["salted 37x53"] if dither else imgs["random 37x53"]
    p = dict(tonemap=tm, transfer=tf, dither=dither, gamma=2.4, white=4.0)
    got8, gotf = D.encode(gpu, img, 0.8, p, want_float=True)
    want8, wantf = D.encode_cpu(gpu, img, 0.8, p, want_float=True)
    assert np.array_equal(got8, want8) and np.array_equal(bits(gotf), bits(wantf))


def test_device_entries_on_a_torch_stream(gpu, imgs):
    """both device entries on a non-default stream, every output pre-filled with a sentinel; with and without the float image"""
    import torch
    for name in ("random 5x7", "random 257x255", "salted 37x53"):
        img = imgs[name]
        h, w = img.shape[:2]
        p = D.DisplayParams(gpu, tonemap="hable", dither=True)
        want_hist = D.histogram_cpu(gpu, img)
        want8, wantf = D.encode_cpu(gpu, img, 1.3, p, want_float=True)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            t_rgb = torch.from_numpy(img).cuda()
            t_hist = torch.full((A.FTN_DISPLAY_HIST_WORDS,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
            t_8 = torch.full((h, w), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
            t_8b = torch.full((h, w), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
            t_f = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
            D.histogram_device(gpu, t_rgb.data_ptr(), w, h, t_hist.data_ptr(), s.cuda_stream)
            D.encode_device(gpu, t_rgb.data_ptr(), w, h, 1.3, t_f.data_ptr(), t_8.data_ptr(), s.cuda_stream, p)
            D.encode_device(gpu, t_rgb.data_ptr(), w, h, 1.3, None, t_8b.data_ptr(), s.cuda_stream, p)
        s.synchronize()
        assert np.array_equal(t_hist.cpu().numpy().view(np.uint32), want_hist), name
        assert np.array_equal(t_8.cpu().numpy().view(np.uint32), want8) and np.array_equal(t_8b.cpu().numpy().view(np.uint32), want8), name
        assert np.array_equal(bits(t_f.cpu().numpy()), bits(wantf)), name
        assert np.array_equal(bits(t_rgb.cpu().numpy()), bits(img))


def test_graph_capture(gpu, imgs):
    """ftn_display_histogram_device then ftn_display_encode_device captured once in a torch.cuda.graph on one stream (every buffer
    allocated before the capture; the histogram's clear is part of it), replayed twice with new inputs copied into the captured buffer"""
    import torch
    img = imgs["random 257x255"]
    h, w = img.shape[:2]
    rng = np.random.default_rng(2)
    inputs = [img, (img * rng.uniform(0.25, 4.0, img.shape)).astype(F32)]
    p = D.DisplayParams(gpu, tonemap="reinhard", dither=True)
    t_rgb = torch.from_numpy(img).cuda()
    t_hist = torch.zeros(A.FTN_DISPLAY_HIST_WORDS, dtype=torch.int32, device="cuda")
    t_8 = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    t_f = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")

    def run():
        stream = torch.cuda.current_stream().cuda_stream
        D.histogram_device(gpu, t_rgb.data_ptr(), w, h, t_hist.data_ptr(), stream)
        D.encode_device(gpu, t_rgb.data_ptr(), w, h, 0.6, t_f.data_ptr(), t_8.data_ptr(), stream, p)

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
        t_hist.fill_(7)                                                  # the captured clear must undo this
        t_8.fill_(0)
        t_f.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        want8, wantf = D.encode_cpu(gpu, r, 0.6, p, want_float=True)
        assert np.array_equal(t_hist.cpu().numpy().view(np.uint32), D.histogram_cpu(gpu, r))
        assert np.array_equal(t_8.cpu().numpy().view(np.uint32), want8) and np.array_equal(bits(t_f.cpu().numpy()), bits(wantf))


@pytest.fixture(scope="module")
def cornell(gpu):
    from fountain_amd import PathIntegrator, RandomSampler, scenes
    b, cam, res = scenes.cornell(gpu, res=32)
    rgb, _, _, _ = scenes.render(gpu, b, cam, res, PathIntegrator(5, 1.0), RandomSampler(4, 0, indexed=True))
    return np.ascontiguousarray(rgb, dtype=F32)


def test_whole_chain_on_a_rendered_cornell_box(gpu, cornell):
    """ftn_display in automatic mode against the chain of the twins; the exposure against the float64 restatement; repeated calls give
    the same bits and leave the input alone"""
    before = cornell.copy()
    for p in (dict(auto_exposure=True), dict(auto_exposure=True, tonemap="hable", dither=True, key=0.3), dict(ev=1.5)):
        got8, gotf, info = D.display(gpu, cornell, p, want_float=True)
        want8, wantf, winfo = D.display_cpu(gpu, cornell, p, want_float=True)
        assert info == winfo
        assert np.array_equal(got8, want8) and np.array_equal(bits(gotf), bits(wantf))
        again8, againf, ainfo = D.display(gpu, cornell, p, want_float=True)
        assert np.array_equal(again8, got8) and np.array_equal(bits(againf), bits(gotf)) and ainfo == info
    info = D.display(gpu, cornell, dict(auto_exposure=True))[1]
    scale, avg, empty = R.exposure64(R.histogram(cornell))
    assert not empty and info["count_bins"] > 0 and abs(float(info["scale"]) - float(F32(scale))) <= float(np.spacing(F32(scale)))
    assert abs(info["avg_log2"] - avg) <= 1e-12 * max(1.0, abs(avg))
    assert np.array_equal(bits(cornell), bits(before))
    codes, _ = R.unpack(D.display(gpu, cornell, dict(auto_exposure=True))[0])
    assert 20 < codes.mean() < 235                                      # an exposed picture, neither black nor burnt out


@pytest.mark.parametrize("name", ["random 1x1", "random 37x53"])
def test_whole_chain_with_and_without_its_optional_buffers(gpu, imgs, name):
    """ftn_display on images of one pixel and of no whole tile: with the automatic exposure (a histogram on the device) and without
    (none), with the float image and without, each against the chain of the twins"""
    img = imgs[name]
    for p in (dict(auto_exposure=True), dict(ev=-0.5, dither=True)):
        want8, wantf, winfo = D.display_cpu(gpu, img, p, want_float=True)
        got8, gotf, info = D.display(gpu, img, p, want_float=True)
        assert np.array_equal(got8, want8) and np.array_equal(bits(gotf), bits(wantf)) and info == winfo, (name, p)
        got8, info = D.display(gpu, img, p)
        assert np.array_equal(got8, want8) and info == winfo, (name, p)


def test_cli(gpu, tmp_path):
    """--png --auto-exposure --denoise writes out.png and out_denoised.png, both encoded at the main image's exposure and readable by
    the independent reader; the OpenEXR files beside them are byte for byte those written without --png; fountain_amd.display converts
    the written file to the same picture"""
    from fountain_amd import render
    from fountain_amd.api import read_exr
    scene_file = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")
    plain, out = tmp_path / "plain", tmp_path / "png"
    plain.mkdir()
    out.mkdir()
    assert render.main([scene_file, "-o", str(plain / "out.exr"), "--samples", "4", "--denoise"]) == 0
    assert render.main([scene_file, "-o", str(out / "out.exr"), "--samples", "4", "--denoise", "--png", "--auto-exposure"]) == 0
    assert sorted(p.name for p in plain.iterdir()) == ["out.exr", "out_denoised.exr"]
    assert sorted(p.name for p in out.iterdir()) == ["out.exr", "out.png", "out_denoised.exr", "out_denoised.png"]
    for name in ("out.exr", "out_denoised.exr"):
        assert (plain / name).read_bytes() == (out / name).read_bytes(), name
    main, den = read_exr(str(out / "out.exr"), gpu), read_exr(str(out / "out_denoised.exr"), gpu)
    scale = D.exposure(gpu, D.histogram_cpu(gpu, main), dict(auto_exposure=True))["scale"]
    for name, img in (("out.png", main), ("out_denoised.png", den)):
        png = R.read_png(str(out / name))
        assert png["chunks"] == ["IHDR", "sRGB", "IDAT", "IEND"] and (png["width"], png["height"]) == (img.shape[1], img.shape[0])
        want, _ = R.unpack(D.encode_cpu(gpu, img, scale))                   # both at the exposure of the main image
        assert np.array_equal(png["pixels"].astype(np.int64), want), name
    assert D.main([str(out / "out.exr"), "-o", str(tmp_path / "conv.png"), "--auto-exposure"]) == 0
    assert np.array_equal(R.read_png(str(tmp_path / "conv.png"))["pixels"], R.read_png(str(out / "out.png"))["pixels"])
