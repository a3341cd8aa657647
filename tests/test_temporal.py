"""Temporal reprojection and accumulation on the GPU (include/fountain_hip_temporal.h, fountain_amd/temporal.py): the device path equals the
host twin bit for bit on synthetic frames, on the edge inputs, on rendered Cornell frames of two cameras and on a size that takes the
tile loop round twice; ftn_temporal_accumulate_device on a torch stream and in a captured graph; eight 4-sample frames of an indexed
sampler are one 32-sample render; quality against converged renders under a static and under a moving camera; the CLI."""
import os

import numpy as np
import pytest

from fountain_amd import _abi as A
from fountain_amd import PathIntegrator, PerspectiveCamera, RandomSampler, scenes
from fountain_amd import denoise as D
from fountain_amd import gbuffer as G
from fountain_amd import moments as M
from fountain_amd import temporal as T

import _temporal_ref as R
import test_denoise as TD
import test_temporal_cpu as TC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = TC.bits
# accumulated + guided against guided alone on the last of eight 4-spp Cornell frames of a moving camera, relative MSE against 1024 spp:
# the measured ratio (profiles/temporal/sweep.json) and the test's bound, that ratio with a margin of a quarter
MOVING_RATIO_MEASURED = 0.8749
MOVING_RATIO_BOUND = min(1.0, 1.25 * MOVING_RATIO_MEASURED)


def same_bits(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def run_both(gpu, cams, frames, params, origin=(0, 0)):
    """a sequence on the device and on the twin, each fed its own history; returns the device's per-frame outputs"""
    h, w = frames[0][0].shape[:2]
    film = R.film_desc(A, (w, h), origin, full=(w + origin[0] + 3, h + origin[1] + 2))
    prev_d = prev_c = None
    out = []
    for cam, fr in zip(cams, frames):
        desc = R.camera_desc(A, cam)
        dev = T.temporal_accumulate(gpu, *fr, desc, film, prev_d, params)
        cpu = T.temporal_accumulate_cpu(gpu, *fr, desc, film, prev_c, params)
        assert same_bits(dev, cpu)
        prev_d, prev_c = (desc, fr[1], dev[0]), (desc, fr[1], cpu[0])
        out.append(dev)
    return out


# ------------------------------------------------------------------ 1. device equals twin
@pytest.mark.parametrize("h,w", TC.SIZES)
def test_synthetic_device_equals_twin(gpu, h, w):
    for motion in (0.3, 4.7):
        cams, frames = TC.sequence(h, w, motion, seed=1000 * h + w)
        for p, origin in ((dict(flags=0, alpha_min=0.0, normal_tol=0.05, plane_tol=0.004), (7, 3)), (dict(flags=1, alpha_min=0.2), (0, 0)), (None, (0, 0)),
                          (dict(alpha_min=0.0, normal_tol=4.0, plane_tol=0.01, albedo_tol=1.0), (0, 0))):
            out = run_both(gpu, cams, frames, p, origin)
    if h * w > 1000:
        assert (out[-1][0][..., 3] > 2).mean() > 0.5


def test_edge_inputs_device_equals_twin(gpu):
    """the edge inputs of tests/test_temporal_cpu.py: non-finite colours, NaN, negative and infinite variances, non-finite positions and
    normals, spoiled history (n = 0, NaN n, non-finite colours and variances), no-history cameras, sky under a rotation, thin images"""
    cams, frames = TC.edge_case_inputs()
    h, w = frames[0][0].shape[:2]
    film = R.film_desc(A, (w, h))
    d = [R.camera_desc(A, c) for c in cams]
    for flags in (0, 1):
        p = dict(flags=flags, normal_tol=0.05, plane_tol=0.004)
        hist0 = TC.spoil_history(T.temporal_accumulate(gpu, *frames[0], d[0], film, None, p)[0])
        prev = (d[0], frames[0][1], hist0)
        assert same_bits(T.temporal_accumulate(gpu, *frames[1], d[1], film, prev, p), T.temporal_accumulate_cpu(gpu, *frames[1], d[1], film, prev, p))
        for cam in (R.pinhole((40.0, 0, -1.0), (w, h), 48.0), R.pinhole((0, 0, 10.0), (w, h), 48.0), R.pinhole((0, 0, 2.0), (w, h), 48.0)):
            prev = (R.camera_desc(A, cam), frames[0][1], hist0)
            got = T.temporal_accumulate(gpu, *frames[1], d[1], film, prev, p)
            assert same_bits(got, T.temporal_accumulate_cpu(gpu, *frames[1], d[1], film, prev, p))
    sky = [R.pinhole((0, 0, 0), (64, 48), 50.0), R.pinhole((0, 0, 0), (64, 48), 50.0, yaw=2.3 / 50, pitch=0.6 / 50)]
    out = run_both(gpu, sky, [R.make_frame(c, [], 48, 64, seed=k) for k, c in enumerate(sky)], dict(alpha_min=0.0))
    assert (out[1][0][4:-4, 4:-4, 3] == 2).all()
    for h, w in ((1, 40), (40, 1)):
        thin = [R.pinhole((0, 0, -1.0), (w, h), 30.0), R.pinhole((0.1, 0.1, -1.0), (w, h), 30.0, yaw=0.01)]
        run_both(gpu, thin, [R.make_frame(c, TC.TWO_PLANES, h, w, seed=k) for k, c in enumerate(thin)], None)
    cam, still = TC.silhouette_sequence()                                                         # equal cameras: no geometry tests
    out = run_both(gpu, [cam] * len(still), still, dict(alpha_min=0.0))
    assert (out[-1][0][..., 3] == len(still)).mean() > 0.95
    one = R.make_frame(sky[0], [], 48, 64, seed=4, spp=1)                                         # 1 sample: var4 = +inf everywhere
    out = run_both(gpu, [sky[0]] * 2, [one, one], None)
    assert np.isinf(out[1][2]).all() and (out[1][0][..., 3] == 2).all()


@pytest.mark.parametrize("h,w", [(1, 1), (53, 37)])
def test_host_history_need_not_be_aligned(gpu, h, w):
    """the host-buffer entry takes a previous history at any 4-byte address (only device pointers need 16): a first frame, then a second
    one whose previous history starts 4, 8 and 12 bytes past a 16-byte boundary, device against twin and against the aligned call"""
    cams, frames = TC.sequence(h, w, 0.3, seed=1000 * h + w)
    film = R.film_desc(A, (w, h))
    d = [R.camera_desc(A, c) for c in cams]
    first = T.temporal_accumulate(gpu, *frames[0], d[0], film, None, None)
    assert same_bits(first, T.temporal_accumulate_cpu(gpu, *frames[0], d[0], film, None, None))
    aligned = T.temporal_accumulate(gpu, *frames[1], d[1], film, (d[0], frames[0][1], first[0]), None)
    raw = np.zeros(first[0].size + 8, np.float32)
    at = (-raw.ctypes.data // 4) % 4                                     # floats up to the next 16-byte boundary
    for off in (1, 2, 3):
        hist = raw[at + off:at + off + first[0].size].reshape(first[0].shape)
        hist[...] = first[0]
        assert hist.ctypes.data % 16 == 4 * off and hist.flags["C_CONTIGUOUS"]
        prev = (d[0], frames[0][1], hist)
        got = T.temporal_accumulate(gpu, *frames[1], d[1], film, prev, None)
        assert same_bits(got, T.temporal_accumulate_cpu(gpu, *frames[1], d[1], film, prev, None)) and same_bits(got, aligned)


def arc_camera(be, k, n=8, res=128, step=0.01):
    """camera k of n on a short arc around the Cornell box that ends at scenes.cornell's own camera: `step` radians a frame, about 1.8
    pixels at the box's centre at 128^2"""
    t = (k - (n - 1)) * step
    return PerspectiveCamera.look_at(be, (3.4 * np.sin(t), -3.4 * np.cos(t), 0.0), (0, 0, 0), (0, 0, 1), (res, res), fov=40.0)


def render_frame(be, scene, cam, res, sampler):
    """(rgb, gb12, var4, film) of one frame: beauty and variance from render_moments, the G-buffer of the same camera samples"""
    var4, film, _, _ = M.render_moments(be, None, cam, res, PathIntegrator(5, 1.0), sampler, scene=scene)
    rgb, _ = film.into_spectrum_buffer()
    r, _, _ = G.render_gbuffer(be, None, cam, res, sampler, scene=scene)
    return rgb, np.concatenate([r[k] for k in G.CHANNELS], axis=-1), var4, film


@pytest.fixture(scope="module")
def cornell(gpu):
    """the Cornell box at 128^2: the scene, eight 4-spp frames on the arc (seed k), and the 1024-spp image at the last camera"""
    b, cam, res = scenes.cornell(gpu, res=128)
    scene = b.create_scene()
    cams = [arc_camera(gpu, k) for k in range(8)]
    frames = [render_frame(gpu, scene, c, res, RandomSampler(4, 100 + k, indexed=True)) for k, c in enumerate(cams)]
    ref, _, _, _ = scenes.render(gpu, None, cam, res, PathIntegrator(5, 1.0), RandomSampler(1024, 77, indexed=True), scene=scene)
    return dict(scene=scene, cam=cam, res=res, cams=cams, frames=frames, ref=ref)


def test_rendered_device_equals_twin(gpu, cornell):
    """two rendered frames of two look_at cameras, both flags; the second frame finds history nearly everywhere"""
    (f0, f1), (c0, c1) = cornell["frames"][6:8], cornell["cams"][6:8]
    for flags in (0, 1):
        p = dict(flags=flags)
        first = T.temporal_accumulate(gpu, *f0[:3], c0, f0[3], None, p)
        assert same_bits(first, T.temporal_accumulate_cpu(gpu, *f0[:3], c0, f0[3], None, p))
        prev = (c0, f0[1], first[0])
        got = T.temporal_accumulate(gpu, *f1[:3], c1, f1[3], prev, p)
        assert same_bits(got, T.temporal_accumulate_cpu(gpu, *f1[:3], c1, f1[3], prev, p))
        assert np.isfinite(got[1]).all() and (got[0][..., 3] > 1).mean() > 0.8


def test_tile_loop_goes_round_twice(gpu):
    """k_tp_accumulate runs at most 65536 workgroups of one 16 x 16 tile: 4112^2 pixels are 66049 tiles.  One plane at distance 3 over
    x <= 1 with sky beside it, written directly in binary32; both frames share the G-buffer (the plane does not move, and a frame's
    positions need not be its pixel centres), the camera moves by about 2 pixels and turns by 3."""
    h = w = 4112
    f = 3000.0
    rng = np.random.default_rng(5)
    cams = [R.pinhole((0, 0, -1.0), (w, h), f), R.pinhole((0.002, -0.001, -1.0), (w, h), f, yaw=1e-3)]
    gb = np.zeros((h, w, 12), np.float32)
    X = ((np.arange(w) + 0.5 - w / 2) * (3.0 / f) + 0.002).astype(np.float32)
    gb[..., 0:3], gb[..., 5], gb[..., 6], gb[..., 8], gb[..., 9], gb[..., 10] = 0.5, -1.0, X[None, :], 2.0, 3.0, 1.0
    gb[..., 7] = ((np.arange(h) + 0.5 - h / 2) * (3.0 / f) - 0.001).astype(np.float32)[:, None]
    gb[:, X > 1.0] = 0.0
    gb[..., 11] = 2.0
    assert (gb[..., 10] == 0).any() and (gb[..., 10] == 1).any()
    mk = lambda k, scale: (rng.random((h, w, k), dtype=np.float32) + np.float32(0.1)) * np.float32(scale)
    frames = [(mk(3, 1.0), gb, mk(4, 0.01)), (mk(3, 1.0), gb, mk(4, 0.01))]
    out = run_both(gpu, cams, frames, None)
    n = out[1][0][..., 3]
    # the last row of tiles is past the first trip; a few columns at the plane's edge and the border the move brought in find no history
    assert (n[-16:-8, 16:-16] == 2).mean() > 0.99 and (n[8:16, 16:-16] == 2).mean() > 0.99 and (n == 2).mean() > 0.99


# ------------------------------------------------------------------ 2. torch stream, graphs, inputs
def test_torch_stream_graph_and_inputs(gpu, cornell):
    """caller buffers on a side stream, then the same call captured in a graph and replayed for two frame pairs: the twin's bits each
    time, the inputs untouched"""
    import torch
    from fountain_amd import FountainError
    fr, cams = cornell["frames"], cornell["cams"]
    film = fr[0][3]
    h, w = fr[0][0].shape[:2]
    hist0 = T.temporal_accumulate_cpu(gpu, *fr[0][:3], cams[0], film)[0]
    want = T.temporal_accumulate_cpu(gpu, *fr[1][:3], cams[1], film, (cams[0], fr[0][1], hist0))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = [torch.from_numpy(a).cuda() for a in (fr[1][0], fr[1][1], fr[1][2], fr[0][1], hist0)]
        outs = [torch.full((h, w, k), float("nan"), dtype=torch.float32, device="cuda") for k in (8, 3, 4)]
        first = [torch.empty_like(o) for o in outs]
        T.temporal_accumulate_torch(gpu, t[0], t[1], t[2], cams[0], film, *first)                               # a first frame
        T.temporal_accumulate_torch(gpu, t[0], t[1], t[2], cams[1], film, *outs, prev=(cams[0], t[3], t[4]))
    s.synchronize()
    assert same_bits([o.cpu().numpy() for o in outs], want)
    assert same_bits([o.cpu().numpy() for o in first], T.temporal_accumulate_cpu(gpu, *fr[1][:3], cams[0], film))
    for x, a in zip(t, (fr[1][0], fr[1][1], fr[1][2], fr[0][1], hist0)):
        assert np.array_equal(bits(x.cpu().numpy()), bits(a))
    with pytest.raises(ValueError):
        T.temporal_accumulate_torch(gpu, t[0], t[1], t[2][..., :3].contiguous(), cams[1], film, *outs)
    with pytest.raises(ValueError):
        T.temporal_accumulate_torch(gpu, t[0], t[1], t[2], cams[1], film, *outs, prev=(cams[0], t[3]))
    with pytest.raises(FountainError):
        T.temporal_accumulate_torch(gpu, t[0], t[1], t[2], cams[1], film, t[4], outs[1], outs[2], prev=(cams[0], t[3], t[4]))   # in place
    # graph capture: everything allocated before, new inputs copied into the captured buffers
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        T.temporal_accumulate_torch(gpu, t[0], t[1], t[2], cams[1], film, *outs, prev=(cams[0], t[3], t[4]))    # warm-up before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        T.temporal_accumulate_torch(gpu, t[0], t[1], t[2], cams[1], film, *outs, prev=(cams[0], t[3], t[4]))
    scale = np.random.default_rng(2).uniform(0.5, 2.0, (h, w, 1)).astype(np.float32)
    for rgb, var in ((fr[1][0], fr[1][2]), (fr[1][0] * scale, fr[1][2] * scale ** 2)):
        t[0].copy_(torch.from_numpy(rgb))
        t[2].copy_(torch.from_numpy(var))
        for o in outs:
            o.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert same_bits([o.cpu().numpy() for o in outs], T.temporal_accumulate_cpu(gpu, rgb, fr[1][1], var, cams[1], film, (cams[0], fr[0][1], hist0)))


# ------------------------------------------------------------------ 3. eight frames are one render
def test_eight_frames_are_one_render(gpu):
    """Frame k renders samples 4k .. 4k + 3 of an indexed 32-sample sampler, all from one camera, and the frames are accumulated without
    demodulation and with alpha_min = 0: the accumulated image is the mean of the eight frames' means, the 32-sample render the mean of the
    same 32 samples summed in another order.  The scene (test_denoise's yard) shows surfaces and sky.  A pixel whose coverage class is the
    same in all eight frames must reach n = 8 (the tolerances are opened wide: equal cameras, so only the class can refuse a tap; a
    silhouette pixel whose four samples all miss in one frame changes class there and starts afresh, as the header says).

    The bound, with u = 2^-24, m = the largest component of the eight frames' rgb at the pixel and K = 8 frames.  X, Y, Z <= 1.09 m, and a
    row of the XYZ -> RGB matrix sums to at most 5.3 in absolute value, so an error e in the XYZ mean reaches rgb as 5.3 e, and the
    conversion itself (3 products, 2 sums of terms up to 3.6 m) adds about 6 u 3.6 m.  The 32-sample film sums 32 terms in any order,
    31 u per channel mean, and divides: 32 u 1.09 m 5.3 + 22 u m < 210 u m.  A frame sums 4 and divides: (4 1.09 5.3 + 22) u m < 46 u m, and
    the mean of eight such errors is no larger; the recurrence adds at most 3 roundings of values up to m in each of 7 steps, 21 u m.
    Together below 280 u m = 35 K u m; the test allows 40 K u m."""
    b, cam, res = TD._yard(gpu)
    scene = b.create_scene()
    K = 8
    frames = [render_frame(gpu, scene, cam, res, RandomSampler(32, 9, indexed=True, first_sample=4 * k, sample_count=4)) for k in range(K)]
    whole = render_frame(gpu, scene, cam, res, RandomSampler(32, 9, indexed=True))[0]
    cov = np.stack([f[1][..., 10] > 0 for f in frames])
    same = (cov == cov[0]).all(0)
    assert same.mean() > 0.95 and (cov[0] & same).any() and (~cov[0] & same).any()
    acc = T.TemporalAccumulator(gpu, dict(flags=0, alpha_min=0.0, normal_tol=4.0, plane_tol=1e30))
    for f in frames:
        out, _ = acc.push(f[0], f[1], f[2], cam, f[3])
    n = acc.history[..., 3]
    assert (n[same] == K).all()
    m = np.max([np.abs(f[0]).max(-1) for f in frames], axis=0)[..., None]
    err = np.abs(out.astype(np.float64) - whole)
    worst = float((err / (K * 2.0 ** -24 * np.maximum(m, 1e-30)))[same].max())
    print("eight frames against one 32-spp render: worst error %.3g K u m" % worst)
    assert (err[same] <= (40 * K * 2.0 ** -24 * m * np.ones(3))[same]).all()


# ------------------------------------------------------------------ 4. quality
def rel_mse(img, ref):
    return float(np.mean(((img.astype(np.float64) - ref) / (ref + 1e-2)) ** 2))      # tests/test_denoise_guided.py's formula


def test_quality_static_view(gpu, cornell):
    """eight independent 4-spp frames of one camera: the accumulated image's relative MSE would be 1/8 of one frame's for Gaussian noise;
    1/4 is asserted, the factor 2 for the heavy tail of Cornell's noise at 128^2"""
    frames = [render_frame(gpu, cornell["scene"], cornell["cam"], cornell["res"], RandomSampler(4, 200 + k, indexed=True)) for k in range(8)]
    acc = T.TemporalAccumulator(gpu, dict(alpha_min=0.0))
    for f in frames:
        out, ovar = acc.push(f[0], f[1], f[2], cornell["cam"], f[3])
    single = float(np.mean([rel_mse(f[0], cornell["ref"]) for f in frames]))
    got = rel_mse(out, cornell["ref"])
    print("static view, Cornell 128^2, 8 x 4 spp: relative MSE of one frame %.5g, accumulated %.5g (ratio %.4f), mean history length %.2f"
          % (single, got, got / single, float(acc.history[..., 3].mean())))
    assert got <= 0.25 * single
    assert np.median(ovar[..., :3] / np.maximum(frames[-1][2][..., :3], 1e-20)) < 0.25         # the variance the filter will read shrank too


def moving_view_scores(be, frames, cams, ref, params=None, twin=False):
    """(guided alone on the last frame, accumulated + guided on the last frame), relative MSE against `ref`"""
    acc = T.TemporalAccumulator(be, params, cpu=twin)
    for f, c in zip(frames, cams):
        out, ovar = acc.push(f[0], f[1], f[2], c, f[3])
    guided = D.denoise_guided_cpu if twin else D.denoise_guided
    last = frames[-1]
    return rel_mse(guided(be, last[0], last[1], last[2]), ref), rel_mse(guided(be, out, last[1], ovar), ref), rel_mse(out, ref)


def test_quality_moving_view(gpu, cornell):
    """eight cameras on a short arc, 4 spp each: the guided filter over the accumulated image and variance beats the guided filter over
    the last frame alone, both against 1024 spp at the last camera"""
    alone, both, accumulated = moving_view_scores(gpu, cornell["frames"], cornell["cams"], cornell["ref"])
    noisy = rel_mse(cornell["frames"][-1][0], cornell["ref"])
    print("moving view, Cornell 128^2, 8 x 4 spp: relative MSE noisy %.5g, accumulated %.5g, guided alone %.5g, accumulated + guided %.5g (ratio %.4f)"
          % (noisy, accumulated, alone, both, both / alone))
    assert both < alone
    assert both <= MOVING_RATIO_BOUND * alone
    assert accumulated < noisy


# ------------------------------------------------------------------ 5. CLI
def test_cli(gpu, tmp_path):
    from fountain_amd.api import PbrtScene, read_exr
    f0 = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")
    f1 = str(tmp_path / "frame1.pbrt")
    text = open(f0).read()
    assert "LookAt 0 -3.4 0 " in text
    open(f1, "w").write(text.replace("LookAt 0 -3.4 0 ", "LookAt 0.05 -3.4 0.02 "))
    out = str(tmp_path / "out.exr")
    assert T.main([f0, f1, "-o", out, "--samples", "4", "--denoise-guided"]) == 0
    names = ["out_0.exr", "out_0_accumulated.exr", "out_0_denoised_guided.exr", "out_1.exr", "out_1_accumulated.exr", "out_1_denoised_guided.exr"]
    assert sorted(os.listdir(tmp_path)) == sorted(names + ["frame1.pbrt"])
    parsed = [PbrtScene(f, gpu) for f in (f0, f1)]
    scene = parsed[0].create_scene()
    acc = T.TemporalAccumulator(gpu)
    for k, p in enumerate(parsed):
        smp = RandomSampler(4, k, indexed=True)
        var4, film, _, _ = M.render_moments(gpu, None, p.camera, None, PathIntegrator(5, 1.0), smp, scene=scene, film=p.film())
        rgb, _ = film.into_spectrum_buffer()
        r, _, _ = G.render_gbuffer(gpu, None, p.camera, None, smp, scene=scene, film=p.film())
        gb = np.concatenate([r[c] for c in G.CHANNELS], axis=-1)
        o, v = acc.push(rgb, gb, var4, p.camera, film)
        plain, accumulated, denoised = T.frame_paths(out, k)
        assert np.array_equal(bits(read_exr(plain, gpu)), bits(rgb))
        assert np.array_equal(bits(read_exr(accumulated, gpu)), bits(o))
        assert np.array_equal(bits(read_exr(denoised, gpu)), bits(D.denoise_guided(gpu, o, gb, v)))
    assert (acc.history[..., 3] > 1).mean() > 0.8
    plain = str(tmp_path / "plain" / "p.exr")
    os.makedirs(os.path.dirname(plain))
    assert T.main([f0, f1, "-o", plain, "--samples", "2", "--alpha-min", "0.5"]) == 0
    assert sorted(os.listdir(os.path.dirname(plain))) == ["p_0.exr", "p_0_accumulated.exr", "p_1.exr", "p_1_accumulated.exr"]
    assert T.main([f0, f1, "-o", out, "--samples", "1"]) == 2
