"""The reconstruction-filtered film (include/fountain_hip_filter.h) on the GPU.  The device gathers; the host twin, fed with the CPU
oracle's radiance of every camera sample, sums the same terms in the same order: the two agree bit for bit, filter_weight_sum included,
over the films, radii, kinds, crops and tile ranges of test_filter_cpu.py, three integrators, the host and device entry points and a
torch stream.  Then what follows from the order: the pass plan and a repeated call change no bit; split tile ranges stay within the
reordering bound; the box of radius 0.5 equals ftn_render; the statistics; NaN radiance; the command line."""
import os

import numpy as np
import pytest

from fountain_amd import FountainError, PathIntegrator, RandomSampler, SamplerIntegrator, WhittedIntegrator, scenes, _abi as A
from fountain_amd import filters as FL

import _filter_ref as FR
import _gbuffer_ref as GR
import _moments_ref as MR
from test_filter_cpu import CASES, CROP, FULL, INTEGRATORS, make_scene, records, twin
from test_moments_oracle import slit

pytestmark = pytest.mark.gpu
F32 = np.float32
bits = MR.bits
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_scenes = {}


def gpu_scene(gpu, which):
    """the case's scene on the GPU, built once: (scene, camera, resolution)"""
    if which not in _scenes:
        b, cam, res = make_scene(which)(gpu)
        _scenes[which] = (b.create_scene(), cam, res)
    return _scenes[which]


def render(gpu, which, integ, filt, crop, tiles, spp, first, count, seed=17, film=None):
    sc, cam, res = gpu_scene(gpu, which)
    smp = RandomSampler(spp, seed, indexed=True, first_sample=first, sample_count=count)
    _, film, st = FL.render_filtered(gpu, None, cam, res, INTEGRATORS[integ](), smp, filt, tiles=tiles, scene=sc,
                                     film=film or FL.filtered_film(gpu, filt, res, crop))
    return film.pixels, st


def assert_bits(got, want, what=""):
    diff = (bits(got) != bits(want)).any(-1)
    assert not diff.any(), "%s: %d pixels differ, first %r: %r vs %r" % (what, int(diff.sum()), tuple(np.argwhere(diff)[0]), got[tuple(np.argwhere(diff)[0])],
                                                                        want[tuple(np.argwhere(diff)[0])])


@pytest.mark.parametrize("which,integ,kind,radius,crop,tiles,spp,first,count", CASES)
def test_device_against_twin(gpu, orc_det, which, integ, kind, radius, crop, tiles, spp, first, count):
    rec, film = records(orc_det, which, integ, radius, crop, tiles, spp, first, count)
    filt = FL.Filter(kind, radius, be=gpu)
    want = twin(gpu, film, filt, rec)
    got, st = render(gpu, which, integ, filt, crop, tiles, spp, first, count)
    assert_bits(got, want, "%s/%s/%s" % (which, integ, kind))
    assert st["camera_samples"] == len(rec) and want[..., 3].any()


@pytest.mark.parametrize("which,integ,kind,radius,crop,tiles,spp,first,count", [CASES[2], CASES[3], CASES[8], CASES[16]])
def test_device_entry_on_a_torch_stream(gpu, orc_det, which, integ, kind, radius, crop, tiles, spp, first, count):
    """ftn_render_filtered_device adds into a CUDA tensor on the current stream: the twin's film on top of what the tensor held"""
    import torch
    rec, film = records(orc_det, which, integ, radius, crop, tiles, spp, first, count)
    filt = FL.Filter(kind, radius, be=gpu)
    sc, cam, res = gpu_scene(gpu, which)
    f = FL.filtered_film(gpu, filt, res, crop)
    smp = RandomSampler(spp, 17, indexed=True, first_sample=first, sample_count=count)
    start = np.random.default_rng(1).uniform(0, 1, (f.height, f.width, 4)).astype(F32)
    want = (start + twin(gpu, film, filt, rec)).astype(F32)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        px = torch.from_numpy(start).cuda()
        st = FL.render_filtered_torch(sc, cam, f, INTEGRATORS[integ](), smp, filt, px, tiles=tiles)
        got = px.cpu().numpy()
    stream.synchronize()
    assert_bits(got, want, "%s/%s device entry" % (which, kind))
    assert st["camera_samples"] == len(rec)


def test_pass_plan_changes_no_bit(gpu, monkeypatch):
    """FTN_WF_PATHS_M=1 on the slit film (12992 x 2: 813 tiles at radius 1.25, five samples a pass, so [3, 10) of 20 runs as two passes
    whose edges fall off the gather's chunk) equals the single-plan result bit for bit: s is the outer loop of every pixel's sum"""
    b, cam, res = slit(gpu)
    sc = b.create_scene()
    filt = FL.Filter("gaussian", (1.25, 1.25), be=gpu)
    smp = RandomSampler(20, 17, indexed=True, first_sample=3, sample_count=7)
    _, one, st1 = FL.render_filtered(gpu, None, cam, res, PathIntegrator(1, 1.0), smp, filt, scene=sc)
    monkeypatch.setenv("FTN_WF_PATHS_M", "1")
    _, two, st2 = FL.render_filtered(gpu, None, cam, res, PathIntegrator(1, 1.0), smp, filt, scene=sc)
    monkeypatch.delenv("FTN_WF_PATHS_M")
    assert_bits(two.pixels, one.pixels, "chunked")
    assert st1["camera_samples"] == st2["camera_samples"] == 7 * (12992 + 2) * (2 + 2) and one.pixels[..., 3].all() and one.pixels[..., :3].any()


def test_split_tile_ranges_and_repeats(gpu, orc_det):
    """the same call twice: equal bits.  Two calls over complementary tile ranges into one buffer: each pixel's terms are the one
    call's, cut into two sums that are converted and added separately -- within the bound of the float32 sum against float64, doubled."""
    which, integ, kind, radius, crop, tiles, spp, first, count = CASES[2]
    rec, film = records(orc_det, which, integ, radius, crop, tiles, spp, first, count)
    filt = FL.Filter(kind, radius, be=gpu)
    a, _ = render(gpu, which, integ, filt, crop, None, spp, first, count)
    b, _ = render(gpu, which, integ, filt, crop, None, spp, first, count)
    assert_bits(a, b, "repeat")
    f = FL.filtered_film(gpu, filt, gpu_scene(gpu, which)[2], crop)
    render(gpu, which, integ, filt, crop, (0, 2, 0), spp, first, count, film=f)
    mid = f.pixels.copy()
    render(gpu, which, integ, filt, crop, (1, 2, 0), spp, first, count, film=f)
    ref = FR.film_ref(film, filt.table(), rec)
    FR.assert_within(f.pixels, ref, factor=2.0, what="split")
    assert mid.any() and (bits(mid) != bits(f.pixels)).any() and (bits(f.pixels) != bits(a)).any()      # really two partial films, really another order


def test_box_equals_ftn_render(gpu, orc_det):
    """a box of radius 0.5 through the new entry against ftn_render: equal bits wherever no sample left its own pixel, equal weights
    everywhere, and the same rays"""
    for which, integ, crop, tiles in (("cornell", "path", FULL, None), ("cornell", "direct", CROP, (1, 2, 0)), ("odd", "whitted", FULL, None)):
        rec, film = records(orc_det, which, integ, (0.5, 0.5), crop, tiles, 4, 0, 0)
        own = ~MR.gpu_sums(film, GR.selected_tiles(film, tiles), rec)["foreign"]
        filt = FL.Filter("box", be=gpu)
        got, st = render(gpu, which, integ, filt, crop, tiles, 4, 0, 0)
        sc, cam, res = gpu_scene(gpu, which)
        plain = GR.film(gpu, res, crop)
        st0 = SamplerIntegrator(cam, INTEGRATORS[integ]()).render_parallel(sc, plain, RandomSampler(4, 17, indexed=True), tiles=tiles)
        assert own.sum() >= own.size - 8 and np.array_equal(bits(got[own]), bits(plain.pixels[own])), which
        assert np.array_equal(bits(got[..., 3]), bits(plain.pixels[..., 3]))
        for k in ("rays_closest", "rays_any", "camera_samples", "nodes_visited", "prims_tested"):
            assert st[k] == st0[k], (which, k)


def test_statistics_at_a_wide_radius(gpu):
    """the rays of a filtered call are those of ftn_render over the same film (the true radius decides the tiles and so the samples)"""
    sc, cam, res = gpu_scene(gpu, "cornell")
    filt = FL.Filter("mitchell", be=gpu)
    smp = RandomSampler(4, 17, indexed=True)
    _, _, st = FL.render_filtered(gpu, None, cam, res, PathIntegrator(5, 1.0), smp, filt, scene=sc)
    st0 = SamplerIntegrator(cam, PathIntegrator(5, 1.0)).render_parallel(sc, GR.film(gpu, res, FULL, (2.0, 2.0)), smp)
    for k in ("rays_closest", "rays_any", "camera_samples"):
        assert st[k] == st0[k] and st[k] > 0, k


def test_nan_radiance_and_whitted_lights(gpu):
    """NaN radiance (a NaN-valued emitter on the back wall of the Cornell box: scene data, nothing the device faults on) returns
    ftn_render's code with the film written; Whitted with more than 32 lights is refused before any device work"""
    filt = FL.Filter("gaussian", be=gpu)
    smp = RandomSampler(2, 0, indexed=True)
    nb, ncam, nres = scenes.cornell(gpu, res=16)
    nb.attribute_begin(); nb.material("matte", Kd=(0.0, 0.0, 0.0)); nb.area_light_source("diffuse", L=(float("nan"), 1.0, 1.0))
    scenes._quad(nb, (-0.2, 0.99, -0.2), (0.2, 0.99, -0.2), (0.2, 0.99, 0.2), (-0.2, 0.99, 0.2)); nb.attribute_end()
    nscene = nb.create_scene()
    film = FL.filtered_film(gpu, filt, nres)
    with pytest.raises(FountainError) as e:
        FL.render_filtered(gpu, None, ncam, nres, PathIntegrator(3, 1.0), smp, filt, scene=nscene, film=film)
    assert e.value.code == A.FTN_ERR_NAN_RADIANCE
    assert np.isnan(film.pixels[..., 0]).any() and np.isfinite(film.pixels[..., 3]).all() and (film.pixels[..., 3] > 0).all()
    lb, lcam, lres = scenes.cornell(gpu, res=16)
    for k in range(33):
        lb.light_source("point", I=(1.0, 1.0, 1.0), from_=(0.0, 0.0, 0.01 * k))
    film = FL.filtered_film(gpu, filt, lres)
    with pytest.raises(FountainError) as e:
        FL.render_filtered(gpu, None, lcam, lres, WhittedIntegrator(3), smp, filt, scene=lb.create_scene(), film=film)
    assert e.value.code == A.FTN_ERR_UNSUPPORTED and not film.pixels.any()


def test_cli(gpu, tmp_path):
    """--pixel-filter gaussian writes an image that differs from the plain one; --pixel-filter scene takes the file's statement and
    equals the explicit option; without the option the file's statement changes nothing"""
    from fountain_amd import read_exr, render as R
    golden = os.path.join(ROOT, "tests", "golden", "cornell.pbrt")
    text = open(golden).read()
    assert 'PixelFilter "box"' in text
    with_filter = tmp_path / "gauss.pbrt"
    with_filter.write_text(text.replace('PixelFilter "box"', 'PixelFilter "gaussian" "float xwidth" [1.5] "float ywidth" [1.5]'))
    out = {k: str(tmp_path / (k + ".exr")) for k in ("plain", "plain2", "gauss", "scene", "wide")}
    assert R.main([golden, "-o", out["plain"], "--samples", "2"]) == 0
    assert R.main([str(with_filter), "-o", out["plain2"], "--samples", "2"]) == 0
    assert R.main([golden, "-o", out["gauss"], "--samples", "2", "--pixel-filter", "gaussian", "--filter-width", "1.5"]) == 0
    assert R.main([str(with_filter), "-o", out["scene"], "--samples", "2", "--pixel-filter", "scene"]) == 0
    assert R.main([golden, "-o", out["wide"], "--samples", "2", "--pixel-filter", "gaussian"]) == 0
    img = {k: read_exr(p, gpu) for k, p in out.items()}
    assert np.array_equal(img["plain"], img["plain2"]) and np.array_equal(img["gauss"], img["scene"])
    assert img["gauss"].shape == img["plain"].shape and not np.array_equal(img["gauss"], img["plain"]) and not np.array_equal(img["gauss"], img["wide"])
    assert np.isfinite(img["gauss"]).all() and abs(float(img["gauss"].mean()) / float(img["plain"].mean()) - 1) < 0.1
