"""The variance-guided a-trous denoiser on the GPU (include/fountain_hip_denoise_guided.h, fountain_amd/denoise.py): the device path equals
the host twin bit for bit on synthetic inputs, on a rendered Cornell box and on a textured scene with environment misses (beauty and
variance from render_moments, G-buffer from render_gbuffer), on sizes that take both grid-stride loops round twice and at 4096^2;
ftn_denoise_guided_device on a torch stream and in a captured graph; inputs untouched and repeated calls; quality against converged
renders, on the Cornell box and on a scene whose noise differs by region; the CLI."""
import os

import numpy as np
import pytest

from fountain_amd import PathIntegrator, PerspectiveCamera, RandomSampler, SceneBuilder, scenes
from fountain_amd import denoise as D
from fountain_amd import gbuffer as G
from fountain_amd import moments as M

import _denoise_guided_ref as GR
import test_denoise as TD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = [(1, 1), (3, 0), (5, 1), (5, 0), (10, 1), (10, 0)]        # (levels, flags)
bits = TD.bits


def rendered(be, make, spp, seed=5):
    """(beauty rgb, resolved G-buffer [H, W, 12], variance of the mean [H, W, 4]) of the same camera samples"""
    b, cam, res = make(be)
    scene = b.create_scene()
    smp = RandomSampler(spp, seed, indexed=True)
    var4, film, _, _ = M.render_moments(be, None, cam, res, PathIntegrator(5, 1.0), smp, scene=scene)
    rgb, _ = film.into_spectrum_buffer()
    r, _, _ = G.render_gbuffer(be, None, cam, res, smp, scene=scene)
    return rgb, np.concatenate([r[k] for k in G.CHANNELS], axis=-1), var4


def split_room(be, res=128):
    """Two halves of a floor kept apart by a wall: one lit directly by a point light (little noise), the other only by the bounce off a
    ceiling from a small spherical emitter that a shelf hides from the floor (heavy noise), under a black sky."""
    b = SceneBuilder(be)
    b.light_source("point", I=(8, 8, 8), from_=(-1.5, 1.5, 2.0))
    b.material("matte", Kd=(0.7, 0.7, 0.7))
    scenes._quad(b, (-3, -1, 0), (3, -1, 0), (3, 5, 0), (-3, 5, 0))                                 # floor
    scenes._quad(b, (0, -1, 0), (0, 5, 0), (0, 5, 3), (0, -1, 3))                                   # dividing wall
    scenes._quad(b, (-3, 5, 0), (3, 5, 0), (3, 5, 3), (-3, 5, 3))                                   # back wall
    scenes._quad(b, (0, -1, 3), (0, 5, 3), (3, 5, 3), (3, -1, 3))                                   # ceiling over one half
    scenes._quad(b, (0.2, 0.8, 2.15), (2.8, 0.8, 2.15), (2.8, 3.2, 2.15), (0.2, 3.2, 2.15))         # shelf under the emitter
    b.attribute_begin(); b.material("matte", Kd=(0.0, 0.0, 0.0)); b.area_light_source("diffuse", L=(150.0, 150.0, 150.0))
    b.translate((1.5, 2.0, 2.4)); b.shape("sphere", radius=0.15); b.attribute_end()
    cam = PerspectiveCamera.look_at(be, (0.0, -4.0, 2.0), (0.0, 2.0, 0.6), (0, 0, 1), (res, res), fov=60.0)
    return b, cam, (res, res)


@pytest.fixture(scope="module")
def cornell4(gpu):
    return rendered(gpu, lambda be: scenes.cornell(be, res=128), 4)


@pytest.fixture(scope="module")
def yard4(gpu):
    rgb, gb, var4 = rendered(gpu, TD._yard, 4)
    cov = gb[..., 10]
    assert (cov == 0).any() and (cov == 1).any(), "the scene must show both sky and surfaces"
    return rgb, gb, var4


# ------------------------------------------------------------------ 1. device equals twin
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (9, 17), (48, 64), (120, 200)])
@pytest.mark.parametrize("levels,flags", LEVELS)
def test_synthetic_device_equals_twin(gpu, h, w, levels, flags):
    rgb, gb, var4, _ = GR.synthetic(h, w, seed=1000 * h + w + levels)
    p = dict(levels=levels, flags=flags)
    assert np.array_equal(bits(D.denoise_guided(gpu, rgb, gb, var4, p)), bits(D.denoise_guided_cpu(gpu, rgb, gb, var4, p)))


def test_edge_inputs_device_equals_twin(gpu):
    """non-finite colours and features, NaN, negative and infinite variances, 1 sample (var4 = +inf everywhere), zero variances"""
    rgb, gb, var4, _ = GR.synthetic(48, 64, seed=21)
    rgb[10, 10] = (np.nan, 0.2, 0.3)
    rgb[20, 30] = (np.inf, 1.0, 1.0)
    gb[5, 40, 3] = np.nan
    gb[25, 20, 6] = np.inf
    var4[12, 12, 0] = np.nan
    var4[14, 40, 1] = -1e-3
    var4[30:34, 30:34] = np.inf
    one = GR.synthetic(48, 64, seed=22, samples=1)
    for r, g, v in ((rgb, gb, var4), one[:3], (rgb, gb, np.zeros_like(var4))):
        for p in (dict(flags=0), dict(flags=1), dict(rel_eps=0.0)):
            assert np.array_equal(bits(D.denoise_guided(gpu, r, g, v, p)), bits(D.denoise_guided_cpu(gpu, r, g, v, p)))


@pytest.mark.parametrize("which", ["cornell", "yard"])
@pytest.mark.parametrize("levels,flags", LEVELS)
def test_rendered_device_equals_twin(gpu, cornell4, yard4, which, levels, flags):
    rgb, gb, var4 = {"cornell": cornell4, "yard": yard4}[which]
    p = dict(levels=levels, flags=flags)
    got = D.denoise_guided(gpu, rgb, gb, var4, p)
    assert np.array_equal(bits(got), bits(D.denoise_guided_cpu(gpu, rgb, gb, var4, p)))
    assert np.isfinite(got).all()


def test_rendered_against_float64(gpu, cornell4, yard4):
    """the device on rendered buffers against the float64 restatement of tests/_denoise_guided_ref.py"""
    for rgb, gb, var4 in (cornell4, yard4):
        got = D.denoise_guided(gpu, rgb, gb, var4, dict(levels=3)).astype(np.float64)
        want = GR.reference(rgb, gb, var4, levels=3)
        assert np.array_equal(np.isfinite(got), np.isfinite(want))
        fin = np.isfinite(want)
        err = np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-3)
        assert np.percentile(err, 99.9) <= 1e-4, np.percentile(err, 99.9)


def test_4096_square(gpu):
    rgb, gb, var4, _ = GR.synthetic(4096, 4096, seed=99)
    got = D.denoise_guided(gpu, rgb, gb, var4)
    assert np.array_equal(bits(got), bits(D.denoise_guided_cpu(gpu, rgb, gb, var4)))


@pytest.mark.parametrize("h,w", [(4112, 4112), (1, 1048592), (1048592, 1)])
def test_grid_stride_loops(gpu, h, w):
    """k_dn_atrous runs at most 65536 workgroups of one 16 x 16 tile and k_dng_prepare at most 65536 of 256 pixels: 4112^2 and a row or
    column of 1048592 pixels need a second trip round both loops"""
    rgb, gb, var4, _ = GR.synthetic(h, w, seed=h + 3 * w, samples=2)
    p = dict(levels=2)
    got = D.denoise_guided(gpu, rgb, gb, var4, p)
    assert np.array_equal(bits(got), bits(D.denoise_guided_cpu(gpu, rgb, gb, var4, p)))
    assert np.isfinite(got).all() and not np.array_equal(bits(got), bits(rgb))


def test_zero_levels_on_the_device(gpu):
    import torch
    rgb, gb, var4, _ = GR.synthetic(37, 53, seed=9)
    rgb.reshape(-1)[::7] = np.nan
    rgb.reshape(-1)[3::11] = -np.inf
    for flags in (0, 1):
        p = dict(levels=0, flags=flags)
        assert np.array_equal(bits(D.denoise_guided(gpu, rgb, gb, var4, p)), bits(rgb))
        t = [torch.from_numpy(a).cuda() for a in (rgb, gb, var4)]
        out = torch.full_like(t[0], 7.0)
        D.denoise_guided_torch(gpu, *t, out, params=p)
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(rgb))


# ------------------------------------------------------------------ 2. torch stream, graphs, inputs
def test_torch_stream_and_workspace(gpu, yard4):
    import torch
    from fountain_amd import FountainError
    rgb, gb, var4 = yard4
    want = D.denoise_guided_cpu(gpu, rgb, gb, var4)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t_rgb, t_gb, t_var = (torch.from_numpy(a).cuda() for a in (rgb, gb, var4))
        out = torch.full_like(t_rgb, float("nan"))
        ws = torch.full((D.guided_workspace_bytes(gpu, rgb.shape[1], rgb.shape[0]) // 4,), -1.0, dtype=torch.float32, device="cuda")
        D.denoise_guided_torch(gpu, t_rgb, t_gb, t_var, out, workspace=ws)
        first = out.clone()
        D.denoise_guided_torch(gpu, t_rgb, t_gb, t_var, out)
    s.synchronize()
    assert np.array_equal(bits(first.cpu().numpy()), bits(want))
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    for t, a in ((t_rgb, rgb), (t_gb, gb), (t_var, var4)):
        assert np.array_equal(bits(t.cpu().numpy()), bits(a))
    with pytest.raises(ValueError):
        D.denoise_guided_torch(gpu, t_rgb, t_gb, t_var, out, workspace=ws[:16])
    with pytest.raises(ValueError):
        D.denoise_guided_torch(gpu, t_rgb, t_gb, t_var[..., :3].contiguous(), out)
    with pytest.raises(FountainError):
        D.denoise_guided_torch(gpu, t_rgb, t_gb, t_var, t_rgb)                  # out_rgb overlaps an input


def test_graph_capture(gpu, yard4):
    """ftn_denoise_guided_device captured in a torch.cuda.graph (a workspace allocated before the capture), replayed with new inputs
    copied into the captured buffers"""
    import torch
    rgb, gb, var4 = yard4
    rng = np.random.default_rng(2)
    scale = rng.uniform(0.5, 2.0, rgb.shape[:2] + (1,))
    inputs = [(rgb, gb, var4), ((rgb * scale).astype(np.float32), gb, (var4 * scale ** 2).astype(np.float32))]
    t_rgb, t_gb, t_var = (torch.from_numpy(a).cuda() for a in (rgb, gb, var4))
    out = torch.zeros_like(t_rgb)
    ws = torch.empty(D.guided_workspace_bytes(gpu, rgb.shape[1], rgb.shape[0]), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        D.denoise_guided_torch(gpu, t_rgb, t_gb, t_var, out, workspace=ws)        # warm-up before the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.denoise_guided_torch(gpu, t_rgb, t_gb, t_var, out, workspace=ws)
    for r, f, v in inputs:
        t_rgb.copy_(torch.from_numpy(r))
        t_gb.copy_(torch.from_numpy(f))
        t_var.copy_(torch.from_numpy(v))
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(D.denoise_guided_cpu(gpu, r, f, v)))


def test_host_path_leaves_inputs_and_repeats(gpu, cornell4):
    rgb, gb, var4 = cornell4
    keep = [a.copy() for a in cornell4]
    a = D.denoise_guided(gpu, rgb, gb, var4)
    b = D.denoise_guided(gpu, rgb, gb, var4)
    assert np.array_equal(bits(a), bits(b))
    for x, y in zip(cornell4, keep):
        assert np.array_equal(bits(x), bits(y))


# ------------------------------------------------------------------ 3. quality
def _quality(gpu, make, spp_noisy=4, spp_ref=1024):
    b, cam, res = make(gpu)
    ref, _, _, _ = scenes.render(gpu, b, cam, res, PathIntegrator(5, 1.0), RandomSampler(spp_ref, 77, indexed=True))
    rgb, gb, var4 = rendered(gpu, make, spp_noisy)
    rel = lambda img: float(np.mean(((img.astype(np.float64) - ref) / (ref + 1e-2)) ** 2))
    return rel(rgb), rel(D.denoise(gpu, rgb, gb)), rel(D.denoise_guided(gpu, rgb, gb, var4))


def test_quality_cornell(gpu):
    noisy, unguided, guided = _quality(gpu, lambda be: scenes.cornell(be, res=128))
    print("Cornell 128^2, 4 spp: relative MSE noisy %.5g, unguided %.5g (%.4f), guided %.5g (%.4f)"
          % (noisy, unguided, unguided / noisy, guided, guided / noisy))
    assert guided <= 0.5 * noisy
    assert guided <= 0.5 * unguided                   # measured: 0.025 against 0.253


def test_quality_non_uniform_noise(gpu):
    """direct light next to indirect light only: the guided filter at its defaults beats ftn_denoise at its defaults"""
    noisy, unguided, guided = _quality(gpu, split_room)
    print("split room 128^2, 4 spp: relative MSE noisy %.5g, unguided %.5g (%.4f), guided %.5g (%.4f)"
          % (noisy, unguided, unguided / noisy, guided, guided / noisy))
    assert guided <= 0.5 * unguided                   # measured: 0.115 against 0.687


# ------------------------------------------------------------------ 4. CLI
def test_cli_denoise_guided(gpu, tmp_path):
    from fountain_amd import render
    from fountain_amd.api import PbrtScene, read_exr
    scene_file = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")
    plain, out = str(tmp_path / "plain.exr"), str(tmp_path / "out.exr")
    assert render.main([scene_file, "-o", plain, "--samples", "4"]) == 0
    assert render.main([scene_file, "-o", out, "--samples", "4", "--denoise-guided"]) == 0
    assert sorted(os.listdir(tmp_path)) == ["out.exr", "out_denoised_guided.exr", "plain.exr"]
    img = read_exr(out, gpu)
    assert np.array_equal(bits(img), bits(read_exr(plain, gpu)))
    parsed = PbrtScene(scene_file, gpu)
    scene = parsed.create_scene()
    smp = parsed.sampler(4, indexed=True)
    var4, film, _, _ = M.render_moments(gpu, None, parsed.camera, None, PathIntegrator(5, 1.0), smp, scene=scene, film=parsed.film())
    r, _, _ = G.render_gbuffer(gpu, None, parsed.camera, None, smp, scene=scene, film=parsed.film())
    gb = np.concatenate([r[k] for k in G.CHANNELS], axis=-1)
    assert np.array_equal(bits(read_exr(render.denoised_guided_path(out), gpu)), bits(D.denoise_guided(gpu, img, gb, var4)))
    both = str(tmp_path / "both.exr")
    assert render.main([scene_file, "-o", both, "--samples", "4", "--denoise-guided", "--denoise", "--variance"]) == 0
    for p in (render.denoised_path(both), render.denoised_guided_path(both), render.variance_path(both)):
        assert os.path.exists(p), p
    assert np.array_equal(bits(read_exr(both, gpu)), bits(img))
    assert render.main([scene_file, "-o", str(tmp_path / "x.exr"), "--denoise-guided", "--exact-stream"]) == 2
    assert render.main([scene_file, "-o", str(tmp_path / "x.exr"), "--denoise-guided", "--samples", "1"]) == 2
