"""The a-trous denoiser on the GPU (include/fountain_hip_denoise.h, fountain_amd/denoise.py): the device path equals the host twin bit
for bit on synthetic inputs, on a rendered Cornell box and on a textured scene with environment misses, through ftn_denoise and
through ftn_denoise_device on a torch stream; a 4096^2 image and sizes that take both grid-stride loops round twice; levels = 0 on the
device; a captured graph; the rendered images against the float64 restatement; subnormal weights; the quality against a converged
render; inputs untouched; repeated calls; the CLI."""
import os

import numpy as np
import pytest

from fountain_amd import PathIntegrator, PerspectiveCamera, RandomSampler, SceneBuilder, scenes
from fountain_amd import denoise as D
from fountain_amd import gbuffer as G

import _denoise_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = [(1, 1), (3, 0), (5, 1), (5, 0), (10, 1), (10, 0)]        # (levels, flags)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rendered(be, make, spp, seed=5):
    """(beauty rgb, resolved G-buffer [H, W, 12]) of the same camera samples"""
    b, cam, res = make(be)
    smp = RandomSampler(spp, seed, indexed=True)
    rgb, _, _, scene = scenes.render(be, b, cam, res, PathIntegrator(5, 1.0), smp)
    r, _, _ = G.render_gbuffer(be, None, cam, res, smp, scene=scene)
    return rgb, np.concatenate([r[k] for k in G.CHANNELS], axis=-1)


def _yard(be):
    """a checkerboard floor, a UV-textured wall, matte / plastic / metal spheres under a uniform sky that the camera sees"""
    b = SceneBuilder(be)
    b.light_source("infinite", L=(0.4, 0.5, 0.7))
    b.light_source("point", I=(20, 20, 20), from_=(0.5, -1.0, 3.0))
    b.texture("chk", "spectrum", "checkerboard", uscale=8.0, vscale=8.0, tex1=(0.75, 0.7, 0.6), tex2=(0.15, 0.2, 0.35))
    b.texture("uvt", "spectrum", "uv", uscale=3.0, vscale=2.0)
    b.material("matte", Kd="chk")
    scenes._quad(b, (-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0))
    b.material("matte", Kd="uvt")
    scenes._quad(b, (-4, 3, 0), (4, 3, 0), (4, 3, 1.5), (-4, 3, 1.5))
    b.attribute_begin(); b.material("plastic", Kd=(0.5, 0.1, 0.1), Ks=(0.3, 0.3, 0.3), roughness=0.1); b.translate((-1.0, 0.5, 0.5)); b.shape("sphere", radius=0.5); b.attribute_end()
    b.attribute_begin(); b.material("metal", eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14), roughness=0.2); b.translate((0.8, 1.0, 0.45)); b.shape("sphere", radius=0.45); b.attribute_end()
    b.attribute_begin(); b.material("matte", Kd=(0.3, 0.6, 0.3)); b.translate((0.1, -0.6, 0.3)); b.shape("sphere", radius=0.3); b.attribute_end()
    cam = PerspectiveCamera.look_at(be, (0.3, -3.0, 1.2), (0.0, 1.0, 0.9), (0, 0, 1), (96, 72), fov=65.0)
    return b, cam, (96, 72)


@pytest.fixture(scope="module")
def cornell4(gpu):
    return rendered(gpu, lambda be: scenes.cornell(be, res=128), 4)


@pytest.fixture(scope="module")
def yard4(gpu):
    rgb, gb = rendered(gpu, _yard, 4)
    cov = gb[..., 10]
    assert (cov == 0).any() and (cov == 1).any(), "the scene must show both sky and surfaces"
    return rgb, gb


# ------------------------------------------------------------------ 1. device equals twin
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (9, 17), (48, 64), (120, 200)])
@pytest.mark.parametrize("levels,flags", LEVELS)
def test_synthetic_device_equals_twin(gpu, h, w, levels, flags):
    rgb, gb, _ = R.synthetic(h, w, seed=1000 * h + w + levels)
    p = dict(levels=levels, flags=flags)
    assert np.array_equal(bits(D.denoise(gpu, rgb, gb, p)), bits(D.denoise_cpu(gpu, rgb, gb, p)))


def test_non_finite_device_equals_twin(gpu):
    rgb, gb, _ = R.synthetic(48, 64, seed=21)
    rgb[10, 10] = (np.nan, 0.2, 0.3)
    rgb[20, 30] = (np.inf, 1.0, 1.0)
    rgb[40, 60] = np.nan
    gb[5, 40, 3] = np.nan
    gb[25, 20, 6] = np.inf
    for flags in (0, 1):
        assert np.array_equal(bits(D.denoise(gpu, rgb, gb, dict(flags=flags))), bits(D.denoise_cpu(gpu, rgb, gb, dict(flags=flags))))


@pytest.mark.parametrize("which", ["cornell", "yard"])
@pytest.mark.parametrize("levels,flags", LEVELS)
def test_rendered_device_equals_twin(gpu, cornell4, yard4, which, levels, flags):
    rgb, gb = {"cornell": cornell4, "yard": yard4}[which]
    p = dict(levels=levels, flags=flags)
    got = D.denoise(gpu, rgb, gb, p)
    assert np.array_equal(bits(got), bits(D.denoise_cpu(gpu, rgb, gb, p)))
    assert np.isfinite(got).all()


def test_torch_stream_and_workspace(gpu, yard4):
    """ftn_denoise_device on a non-default stream, with a caller's workspace and with one the wrapper allocates; inputs untouched;
    two calls give the same bits"""
    import torch
    rgb, gb = yard4
    want = D.denoise_cpu(gpu, rgb, gb)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t_rgb = torch.from_numpy(rgb).cuda()
        t_gb = torch.from_numpy(gb).cuda()
        out = torch.full_like(t_rgb, float("nan"))
        ws = torch.full((D.workspace_bytes(gpu, rgb.shape[1], rgb.shape[0]) // 4,), -1.0, dtype=torch.float32, device="cuda")
        D.denoise_torch(gpu, t_rgb, t_gb, out, workspace=ws)
        first = out.clone()
        D.denoise_torch(gpu, t_rgb, t_gb, out)
    s.synchronize()
    assert np.array_equal(bits(first.cpu().numpy()), bits(want))
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    assert np.array_equal(bits(t_rgb.cpu().numpy()), bits(rgb)) and np.array_equal(bits(t_gb.cpu().numpy()), bits(gb))
    with pytest.raises(ValueError):
        D.denoise_torch(gpu, t_rgb, t_gb, out, workspace=ws[:16])
    from fountain_amd import FountainError
    with pytest.raises(FountainError):
        D.denoise_torch(gpu, t_rgb, t_gb, t_rgb)                      # out_rgb overlaps an input


def test_host_path_leaves_inputs_and_repeats(gpu, cornell4):
    rgb, gb = cornell4
    rgb0, gb0 = rgb.copy(), gb.copy()
    a = D.denoise(gpu, rgb, gb)
    b = D.denoise(gpu, rgb, gb)
    assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(rgb), bits(rgb0)) and np.array_equal(bits(gb), bits(gb0))


# ------------------------------------------------------------------ 2. scale
def test_4096_square(gpu):
    rgb, gb, _ = R.synthetic(4096, 4096, seed=99)
    got = D.denoise(gpu, rgb, gb)
    assert np.array_equal(bits(got), bits(D.denoise_cpu(gpu, rgb, gb)))


@pytest.mark.parametrize("h,w", [(4112, 4112), (1, 1048592), (1048592, 1)])
def test_grid_stride_loops(gpu, h, w):
    """k_dn_atrous runs at most 65536 workgroups of one 16 x 16 tile and k_dn_prepare at most 65536 of 256 pixels: 4112^2 (66049
    tiles, more than 2^24 pixels) and a row or column of 1048592 pixels (65537 tiles) need a second trip round both loops"""
    rgb, gb, _ = R.synthetic(h, w, seed=h + 3 * w)
    p = dict(levels=2)
    got = D.denoise(gpu, rgb, gb, p)
    assert np.array_equal(bits(got), bits(D.denoise_cpu(gpu, rgb, gb, p)))
    assert np.isfinite(got).all() and not np.array_equal(bits(got), bits(rgb))


def test_zero_levels_on_the_device(gpu):
    """levels = 0 copies rgb bit for bit, NaN and infinities included, through ftn_denoise and through ftn_denoise_device"""
    import torch
    rgb, gb, _ = R.synthetic(37, 53, seed=9)
    rgb.reshape(-1)[::7] = np.nan
    rgb.reshape(-1)[3::11] = -np.inf
    rgb.reshape(-1)[5::13] = np.inf
    for flags in (0, 1):
        p = dict(levels=0, flags=flags)
        assert np.array_equal(bits(D.denoise(gpu, rgb, gb, p)), bits(rgb))
        t_rgb, t_gb = torch.from_numpy(rgb).cuda(), torch.from_numpy(gb).cuda()
        out = torch.full_like(t_rgb, 7.0)
        D.denoise_torch(gpu, t_rgb, t_gb, out, params=p)
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(rgb))


def test_graph_capture(gpu, yard4):
    """ftn_denoise_device captured in a torch.cuda.graph (one stream, a workspace allocated before the capture), replayed twice with
    new inputs copied into the captured buffers"""
    import torch
    rgb, gb = yard4
    rng = np.random.default_rng(2)
    inputs = [(rgb, gb), ((rgb * rng.uniform(0.5, 2.0, rgb.shape)).astype(np.float32), gb)]
    t_rgb, t_gb = torch.from_numpy(rgb).cuda(), torch.from_numpy(gb).cuda()
    out = torch.zeros_like(t_rgb)
    ws = torch.empty(D.workspace_bytes(gpu, rgb.shape[1], rgb.shape[0]), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        D.denoise_torch(gpu, t_rgb, t_gb, out, workspace=ws)           # warm-up before the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.denoise_torch(gpu, t_rgb, t_gb, out, workspace=ws)
    for r, f in inputs:
        t_rgb.copy_(torch.from_numpy(r))
        t_gb.copy_(torch.from_numpy(f))
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(D.denoise_cpu(gpu, r, f)))


# ------------------------------------------------------------------ 3. against the float64 restatement
@pytest.mark.parametrize("which", ["cornell", "yard"])
@pytest.mark.parametrize("levels,flags", LEVELS)
def test_rendered_device_against_float64(gpu, cornell4, yard4, which, levels, flags):
    """the device on rendered buffers (sky misses with depth inf, partly covered pixels, fireflies) against tests/_denoise_ref.py: the
    non-finite pattern equal, the rest within the first-order binary32 bound the restatement derives"""
    rgb, gb = {"cornell": cornell4, "yard": yard4}[which]
    got = D.denoise(gpu, rgb, gb, dict(levels=levels, flags=flags)).astype(np.float64)
    want, err = R.reference_bound(rgb, gb, levels=levels, flags=flags)
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    fin = np.isfinite(want)
    assert (np.abs(got[fin] - want[fin]) <= err[fin]).all(), "worst error / bound %.3g" % (np.abs(got[fin] - want[fin]) / err[fin]).max()


@pytest.mark.parametrize("t_target,above", [(95.0, False), (104.0, False), (104.0, True)])
def test_subnormal_weights_on_the_device(gpu, t_target, above):
    """the one-tap images of test_denoise_cpu.py on the device: a subnormal weight (t about 95) survives, t = 104 and beyond weigh 0"""
    rgb, gb, p, t, want = R.one_tap(t_target, above)
    got = D.denoise(gpu, rgb, gb, p)
    assert np.array_equal(bits(got[0, 2]), bits(np.full(3, want, np.float32)))
    assert np.array_equal(bits(got), bits(D.denoise_cpu(gpu, rgb, gb, p)))


# ------------------------------------------------------------------ 4. quality
def test_quality_against_a_converged_render(gpu, cornell4):
    rgb, gb = cornell4
    b, cam, res = scenes.cornell(gpu, res=128)
    ref, _, _, _ = scenes.render(gpu, b, cam, res, PathIntegrator(5, 1.0), RandomSampler(1024, 77, indexed=True))
    rel = lambda img: float(np.mean(((img.astype(np.float64) - ref) / (ref + 1e-2)) ** 2))
    noisy, den = rel(rgb), rel(D.denoise(gpu, rgb, gb))
    print("Cornell 128^2, 4 spp: relative MSE noisy %.5g, denoised %.5g, ratio %.4f" % (noisy, den, den / noisy))
    assert den <= 0.5 * noisy


# ------------------------------------------------------------------ 5. CLI
def test_cli_denoise(gpu, tmp_path):
    from fountain_amd import render
    from fountain_amd.api import PbrtScene, read_exr
    scene_file = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")
    plain, out = str(tmp_path / "plain.exr"), str(tmp_path / "out.exr")
    assert render.main([scene_file, "-o", plain, "--samples", "4"]) == 0
    assert render.main([scene_file, "-o", out, "--samples", "4", "--denoise"]) == 0
    assert sorted(os.listdir(tmp_path)) == ["out.exr", "out_denoised.exr", "plain.exr"]
    img = read_exr(out, gpu)
    assert np.array_equal(bits(img), bits(read_exr(plain, gpu)))
    parsed = PbrtScene(scene_file, gpu)
    r, _, _ = G.render_gbuffer(gpu, None, parsed.camera, None, parsed.sampler(4, indexed=True), scene=parsed.create_scene(), film=parsed.film())
    gb = np.concatenate([r[k] for k in G.CHANNELS], axis=-1)
    assert np.array_equal(bits(read_exr(render.denoised_path(out), gpu)), bits(D.denoise(gpu, img, gb)))
    both = str(tmp_path / "both.exr")
    assert render.main([scene_file, "-o", both, "--samples", "4", "--denoise", "--gbuffer"]) == 0
    for p in list(render.gbuffer_paths(both).values()) + [render.denoised_path(both)]:
        assert os.path.exists(p), p
    assert render.main([scene_file, "-o", str(tmp_path / "x.exr"), "--denoise", "--exact-stream"]) == 2
    assert render.main([scene_file, "-o", str(tmp_path / "x.exr"), "--denoise", "--gpus", "2"]) == 2
