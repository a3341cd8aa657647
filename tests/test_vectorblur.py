"""The vector-blur stage on the GPU (include/fountain_hip_vectorblur.h, fountain_amd/vectorblur.py): the device equals the host twin bit for
bit -- the workspace's per-pixel, tile and neighbour records included -- on images of one column, one row, one tile, tiles with ragged
edges and an interior tile, for every motion field, tap count and with and without a G-buffer; the exact copies; the device entry on a
torch stream into NaN-filled buffers and in a captured graph; repeated calls; two rendered frames through the temporal command line and
the standalone command on the files it wrote.  No kernel caps its grid (one workgroup per tile, or per 256 tiles), so no size beyond
80 x 48 is needed."""
import os

import numpy as np
import pytest

from fountain_amd import vectorblur as V

import _vectorblur_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
bits = R.bits


def device_run(gpu, img, m, gb, p, stream=None):
    """vector_blur_device into NaN-filled output and workspace (with four more words behind it) -> (out, the workspace's words, the tail)"""
    import torch
    h, w = img.shape[:2]
    nbytes = V.workspace_size(gpu, w, h)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t_rgb, t_m, t_gb = dev(img), dev(m), dev(gb)
    t_out = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    t_ws = torch.full((nbytes // 4 + 4,), float("nan"), dtype=torch.float32, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())                  # the fills above run on the current stream
    V.vector_blur_device(gpu, t_rgb, t_m, t_gb, t_out, t_ws, stream, p)
    (stream or torch.cuda.current_stream()).synchronize()
    assert np.array_equal(bits(t_rgb.cpu().numpy()), bits(img)) and np.array_equal(bits(t_m.cpu().numpy()), bits(m))
    ws = t_ws.cpu().numpy()
    return t_out.cpu().numpy(), ws[:nbytes // 4], ws[nbytes // 4:]


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
def test_device_equals_twin(gpu, size):
    w, h = size
    img = R.image(w, h)
    for name in R.FIELDS:
        m = R.field(name, w, h)
        for gb in (None, R.gbuffer(w, h)):
            for taps in R.TAPS:
                p = dict(taps=taps)
                want = V.vector_blur_cpu(gpu, img, m, gb, p)
                got = V.vector_blur(gpu, img, m, gb, p)
                assert np.array_equal(bits(got), bits(want)), (size, name, gb is not None, taps, int((bits(got) != bits(want)).sum()))
            # the intermediate arrays, from the device entry's workspace
            out, ws, tail = device_run(gpu, img, m, gb, dict(taps=16))
            assert np.array_equal(bits(out), bits(V.vector_blur_cpu(gpu, img, m, gb, dict(taps=16)))) and np.isnan(tail).all()
            rec, twin = V.split_workspace(ws, w, h), V.velocities_cpu(gpu, m, gb, dict(taps=16))
            for k in ("pixels", "tiles", "neighbours"):
                assert np.array_equal(bits(rec[k]), bits(twin[k])), (size, name, k)
    for p in (dict(shutter=1.0), dict(shutter=0.9, max_radius=9.5, taps=7, depth_extent=0.05), dict(max_radius=0.75, shutter=1.0), dict(depth_extent=1e-6)):
        m, gb = R.field("beyond_clamp", w, h), R.gbuffer(w, h)
        assert np.array_equal(bits(V.vector_blur(gpu, img, m, gb, p)), bits(V.vector_blur_cpu(gpu, img, m, gb, p))), (size, p)


def test_exact_copies_and_non_finite_colours(gpu):
    w, h = 37, 21
    img = R.image(w, h, seed=5)
    flat = img.reshape(-1)
    flat[::29] = np.array([0x7fc12345, 0xffc00001, 0x7f800001, 0x80000000, 0x7f800000, 0xff800000, 0x00000001], np.uint32).view(F32)[np.arange(flat[::29].size) % 7]
    moving = R.field("uniform", w, h)
    for m, p in ((moving, dict(shutter=0.0)), (np.zeros((h, w, 2), F32), {}), (np.full((h, w, 2), np.nan, F32), {}), (np.full((h, w, 2), F32(1.4)), {})):
        for gb in (None, R.gbuffer(w, h)):
            assert np.array_equal(bits(V.vector_blur(gpu, img, m, gb, p)), bits(img))
    got = V.vector_blur(gpu, img, moving, R.gbuffer(w, h))
    assert np.array_equal(bits(got), bits(V.vector_blur_cpu(gpu, img, moving, R.gbuffer(w, h))))
    stays = ~np.isfinite(img).all(-1)
    assert stays.sum() >= 10 and np.array_equal(bits(got[stays]), bits(img[stays])) and np.isfinite(got[~stays]).all()
    one = img[:1, :1]
    assert np.array_equal(bits(V.vector_blur(gpu, one, np.full((1, 1, 2), 30.0, F32))), bits(one))


def test_device_entry_on_a_torch_stream_and_repeated_calls(gpu):
    """ftn_vectorblur_device on a non-default stream, the output and the workspace pre-filled with NaN: a read of either before it is
    written would spread"""
    import torch
    for (w, h), name, with_gb, p in (((80, 48), "rotational", True, dict()), ((17, 33), "beyond_clamp", False, dict(taps=64)), ((1, 7), "uniform", True, dict(taps=2)),
                                     ((48, 48), "fast_tile", True, dict(shutter=1.0))):
        img, m, gb = R.image(w, h), R.field(name, w, h), R.gbuffer(w, h) if with_gb else None
        want = V.vector_blur_cpu(gpu, img, m, gb, p)
        out, ws, tail = device_run(gpu, img, m, gb, p, stream=torch.cuda.Stream())
        assert np.array_equal(bits(out), bits(want)), (w, h, name)
        assert np.isnan(tail).all() and np.isfinite(ws.reshape(-1, 4)[:, :3]).all()       # every record written, nothing behind the workspace
    first = V.vector_blur(gpu, img, m, gb, p)
    assert np.array_equal(bits(V.vector_blur(gpu, img, m, gb, p)), bits(first)) and np.array_equal(bits(first), bits(want))
    with pytest.raises(ValueError):
        V.vector_blur_device(gpu, torch.zeros((4, 4, 3), device="cuda"), torch.zeros((4, 4, 2), device="cuda"), None, torch.zeros((4, 4, 3), device="cuda"),
                             torch.zeros(4, device="cuda"))                                  # a workspace too small


def test_graph_capture(gpu):
    """ftn_vectorblur_device captured once in a torch.cuda.graph (every buffer allocated before the capture), replayed twice with new
    inputs copied into the captured buffers"""
    import torch
    w, h = 80, 48
    img, m, gb = R.image(w, h), R.field("rotational", w, h), R.gbuffer(w, h)
    inputs = [(R.image(w, h, seed=9), R.field("beyond_clamp", w, h, seed=4)), (R.image(w, h, seed=10), R.field("uniform", w, h))]
    t_rgb, t_m, t_gb = (torch.from_numpy(a).cuda() for a in (img, m, gb))
    t_out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    t_ws = torch.zeros(V.workspace_size(gpu, w, h) // 4, dtype=torch.float32, device="cuda")
    run = lambda: V.vector_blur_device(gpu, t_rgb, t_m, t_gb, t_out, t_ws)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                                            # warm-up before the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for r, mv in inputs:
        t_rgb.copy_(torch.from_numpy(r))
        t_m.copy_(torch.from_numpy(mv))
        t_out.fill_(float("nan"))
        t_ws.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(t_out.cpu().numpy()), bits(V.vector_blur_cpu(gpu, r, mv, gb)))


def test_cli(gpu, tmp_path):
    """two frames of tests/test_motion.py's command-line scene (the sphere and the camera moved) through `temporal --dynamic
    --vector-blur`: out_1_blurred.exr is vector_blur of the same renders bit for bit, differs from out_1.exr where the sphere moved and
    equals it in every tile whose neighbour maximum is at most half a pixel; no frame 0 file; without the option the files of before, byte
    for byte; the standalone command on the written files"""
    from fountain_amd import PbrtScene, RandomSampler, read_exr, write_exr
    from fountain_amd import gbuffer as G
    from fountain_amd import temporal as T
    from test_motion import FRAME
    files = []
    for k, (eye, x) in enumerate(((0.0, -0.6), (0.2, 0.6))):             # (twice that test's step of the sphere: a blur of several pixels)
        files.append(tmp_path / ("f%d.pbrt" % k))
        files[-1].write_text(FRAME % (eye, x))
    plain, out = tmp_path / "plain" / "o.exr", tmp_path / "blur" / "o.exr"
    os.makedirs(plain.parent)
    os.makedirs(out.parent)
    args = [str(f) for f in files] + ["--samples", "4", "--dynamic"]
    assert T.main(args + ["-o", str(plain)]) == 0
    assert T.main(args + ["-o", str(out), "--vector-blur", "1.0"]) == 0
    before = ["o_0.exr", "o_0_accumulated.exr", "o_1.exr", "o_1_accumulated.exr", "o_1_motion.exr"]
    assert sorted(os.listdir(plain.parent)) == before and sorted(os.listdir(out.parent)) == sorted(before + ["o_1_blurred.exr"])
    for name in before:
        assert (plain.parent / name).read_bytes() == (out.parent / name).read_bytes(), name
    img = read_exr(str(out.parent / "o_1.exr"), gpu)
    mv = read_exr(str(out.parent / "o_1_motion.exr"), gpu)[..., :2]
    blurred = read_exr(str(out.parent / "o_1_blurred.exr"), gpu)
    fr = PbrtScene(str(files[1]), gpu)
    r, _, _ = G.render_gbuffer(gpu, None, fr.camera, None, RandomSampler.new_with_seed(4, 1, indexed=True), scene=fr.create_scene(), film=fr.film())
    gb12 = np.ascontiguousarray(np.concatenate([r[c] for c in G.CHANNELS], axis=-1))
    p = dict(shutter=1.0)
    assert np.array_equal(bits(blurred), bits(V.vector_blur(gpu, img, mv, gb12, p))) and np.array_equal(bits(blurred), bits(V.vector_blur_cpu(gpu, img, mv, gb12, p)))
    h, w = img.shape[:2]
    changed = (bits(blurred) != bits(img)).any(-1)
    with np.errstate(invalid="ignore"):
        speed = np.where(np.isfinite(mv).all(-1), np.hypot(mv[..., 0], mv[..., 1]), 0.0)
    fast = speed > 4.0                                                                     # the sphere: a half velocity above 2 pixels
    print("the largest motion is %.2f pixels, %d pixels above 4" % (speed.max(), fast.sum()))
    assert fast.sum() >= 8 and changed[fast].mean() > 0.5                                  # (the sphere covers about a dozen of the 24 x 16 pixels)
    nb = V.velocities_cpu(gpu, mv, gb12, p)["neighbours"][..., 2]
    still = np.repeat(np.repeat(nb <= 0.25, R.TILE, axis=0), R.TILE, axis=1)[:h, :w]
    assert not changed[still].any()
    # the flag alone: the default shutter
    os.makedirs(tmp_path / "d")
    assert T.main(args + ["-o", str(tmp_path / "d" / "o.exr"), "--vector-blur"]) == 0
    assert np.array_equal(bits(read_exr(str(tmp_path / "d" / "o_1_blurred.exr"), gpu)), bits(V.vector_blur_cpu(gpu, img, mv, gb12)))
    # the standalone command: the same picture from the files, without a depth file and with one
    assert V.main([str(out.parent / "o_1.exr"), "--motion", str(out.parent / "o_1_motion.exr"), "--shutter", "1.0", "-o", str(tmp_path / "a.exr")]) == 0
    assert np.array_equal(bits(read_exr(str(tmp_path / "a.exr"), gpu)), bits(V.vector_blur_cpu(gpu, img, mv, None, p)))
    depth = np.where(gb12[..., 10] > 0, gb12[..., 9], F32(0))                            # 0 where nothing was hit: background to the command
    write_exr(str(tmp_path / "depth.exr"), np.repeat(depth[..., None], 3, axis=-1), gpu)
    assert V.main([str(out.parent / "o_1.exr"), "--motion", str(out.parent / "o_1_motion.exr"), "--depth", str(tmp_path / "depth.exr"), "--taps", "9",
                   "--max-radius", "6", "-o", str(tmp_path / "b.exr")]) == 0
    want = V.vector_blur_cpu(gpu, img, mv, V.gb12_from_depth(depth), dict(taps=9, max_radius=6.0))
    assert np.array_equal(bits(read_exr(str(tmp_path / "b.exr"), gpu)), bits(want))
    assert V.main([str(out.parent / "o_1.exr"), "--motion", str(out.parent / "o_1_motion.exr")]) == 0        # the default name and parameters
    assert np.array_equal(bits(read_exr(str(out.parent / "o_1_blurred.exr"), gpu)), bits(V.vector_blur_cpu(gpu, img, mv)))
