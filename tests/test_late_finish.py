"""Late finish (FTN_WF_LATE_FINISH): in an environment-lit scene the path integrator's wavefront no longer queues an
ended path again for its pending direct term, and k_wf_classify drops the paths whose ray escaped or that reached max_depth; every path
leaves one record and k_wf_accumulate adds what its radiance still needs (wf_finish_path: the source k_wf_shade runs).  That moves
additions to another kernel, never changes one: knob on (the default) against knob off gives the same film bit for bit and the same
counts, at every place where the new route differs from the old one -- the first pass, the end of the bounce loop, the accumulate
kernel's chunks and clipped tiles, several passes, the hooks that read a pass's radiance -- and the default equals the oracle.

An assertion error here names a kernel bug: a film difference with equal counts points at wf_finish_path / k_wf_accumulate's staging
(or at a record k_wf_shade did not write), different rays_any at the any-hit launch behind the bounce loop, different rays_closest at
k_wf_classify's drop mask."""
import numpy as np
import pytest

from fountain_amd import Film, PathIntegrator, PerspectiveCamera, RandomSampler, SamplerIntegrator, SceneBuilder, _abi as A, scenes
from fountain_amd import filters as FL
from fountain_amd import moments as M
from test_gpu_parity import _materials_scene, assert_film_equal, bits

pytestmark = pytest.mark.gpu
WAVE = A.FTN_PIPELINE_WAVEFRONT
COUNTS = ("rays_closest", "rays_any", "camera_samples", "spill_samples")
SMP = RandomSampler(8, 2, indexed=True)


def on_off(monkeypatch, render, env=None):
    """render() -> (arrays, stats) with the knob at its default and at 0 (plus `env` in both): all arrays bit-equal, all counts equal.
    Returns the default's result."""
    out = []
    for k, v in (env or {}).items(): monkeypatch.setenv(k, v)
    for knob in (None, "0"):
        if knob is not None: monkeypatch.setenv("FTN_WF_LATE_FINISH", knob)
        out.append(render())
        if knob is not None: monkeypatch.delenv("FTN_WF_LATE_FINISH")
    for k in (env or {}): monkeypatch.delenv(k)
    (a_on, st_on), (a_off, st_off) = out
    assert {k: st_on[k] for k in COUNTS} == {k: st_off[k] for k in COUNTS}
    assert len(a_on) == len(a_off)
    for i, (x, y) in enumerate(zip(a_on, a_off)):
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), "output plane %d: %d values differ" % (i, int((bits(x) != bits(y)).sum()))
    return out[0]


def beauty(gpu, sc, cam, res, integ, smp):
    def render():
        f = Film(gpu, res)
        st = SamplerIntegrator(cam, integ).render_parallel(sc, f, smp, pipeline=WAVE)
        return (f.pixels,), st
    return render


@pytest.fixture(scope="module")
def cubes(gpu):
    b, cam, res = scenes.instanced_cubes(gpu, n_copies=5, res=(96, 96), env_n=32)
    return b.create_scene(), cam, res


def env_builder(be, n=16, seed=3):
    b = SceneBuilder(be)
    b.light_source("infinite", texels=(np.random.default_rng(seed).random((n, n, 3)) ** 2 * 1.5 + 0.05).astype(np.float32))
    return b


def test_base_case_and_oracle(gpu, orc_det, monkeypatch, cubes):
    """the 5-cube scene at 8 spp, depth 5: knob on = knob off, and the default equals the deterministic oracle (tolerance rule of
    assert_film_equal: last bit of the pixels that received a spill sample)"""
    sc, cam, res = cubes
    (px,), st = on_off(monkeypatch, beauty(gpu, sc, cam, res, PathIntegrator.new(5, 1.0), SMP))
    assert st["rays_any"] > 0 and px[..., :3].any()
    bo, camo, _ = scenes.instanced_cubes(orc_det, n_copies=5, res=(96, 96), env_n=32)
    fo = Film(orc_det, res)
    sto = SamplerIntegrator(camo, PathIntegrator.new(5, 1.0)).render_parallel(bo.create_scene(), fo, SMP)
    assert_film_equal(px, fo.pixels, st["spill_samples"], "late finish vs oracle")
    assert (st["rays_closest"], st["rays_any"], st["camera_samples"]) == (sto["rays_closest"], sto["rays_any"], sto["camera_samples"])


@pytest.mark.parametrize("depth,env", [(0, None), (1, None), (2, None), (1, {"FTN_WF_OVERLAP": "1"})])
def test_the_end_of_the_loop(gpu, monkeypatch, cubes, depth, env):
    """depth 0: the pass behind k_wf_generate is the only one (its launch for the classes without a BSDF writes the records);
    depth 1 and 2: the last round's any-hit launch carries the rays of every path that goes on, also on the side stream"""
    sc, cam, res = cubes
    (px,), st = on_off(monkeypatch, beauty(gpu, sc, cam, res, PathIntegrator.new(depth, 1.0), SMP), env)
    assert px[..., :3].any() and (st["rays_any"] > 0) == (depth > 0)


@pytest.mark.parametrize("spp", [5, 13])
def test_chunk_and_tile_edges(gpu, monkeypatch, spp):
    """5 and 13 samples in a pass (off k_wf_accumulate's chunk of 8) on a 100 x 70 film (tiles clipped at both edges: slots without a path)"""
    b, cam, res = scenes.instanced_cubes(gpu, n_copies=5, res=(100, 70), env_n=32)
    on_off(monkeypatch, beauty(gpu, b.create_scene(), cam, res, PathIntegrator.new(5, 1.0), RandomSampler(spp, 4, indexed=True)))


def test_three_passes(gpu, monkeypatch):
    """37 spp on a 256^2 film with one Mi paths in flight: 16 + 16 + 5 samples over three passes, each leaving its records where the
    last one did"""
    b, cam, res = scenes.instanced_cubes(gpu, n_copies=5, res=(256, 256), env_n=32)
    (px,), st = on_off(monkeypatch, beauty(gpu, b.create_scene(), cam, res, PathIntegrator.new(5, 1.0), RandomSampler(37, 6, indexed=True)), {"FTN_WF_PATHS_M": "1"})
    assert st["camera_samples"] == 256 * 256 * 37


def test_every_path_ends_in_the_first_pass(gpu, monkeypatch):
    """a camera that sees no geometry (the one quad lies behind it): every camera ray escapes, the environment along it is added where
    the first pass writes the record"""
    b = env_builder(gpu)
    b.material("matte", Kd=(0.5, 0.5, 0.5))
    scenes._quad(b, (-1, -9, -1), (1, -9, -1), (1, -9, 1), (-1, -9, 1))
    cam = PerspectiveCamera.look_at(gpu, (0, -5, 0), (0, 0, 0.3), (0, 0, 1), (48, 40), fov=50.0)
    (px,), st = on_off(monkeypatch, beauty(gpu, b.create_scene(), cam, (48, 40), PathIntegrator.new(5, 1.0), SMP))
    assert st["rays_closest"] == st["camera_samples"] and st["rays_any"] == 0 and px[..., :3].all()


def test_no_path_ends_in_the_first_pass(gpu, monkeypatch):
    """a wall of two triangles that fills the view: every camera ray hits, every path goes on"""
    b = env_builder(gpu)
    b.material("matte", Kd=(0.6, 0.5, 0.4))
    scenes._quad(b, (-50, 4, -50), (50, 4, -50), (50, 4, 50), (-50, 4, 50))
    cam = PerspectiveCamera.look_at(gpu, (0, -5, 0), (0, 0, 0), (0, 0, 1), (48, 40), fov=50.0)
    (px,), st = on_off(monkeypatch, beauty(gpu, b.create_scene(), cam, (48, 40), PathIntegrator.new(5, 1.0), SMP))
    assert st["rays_closest"] >= 2 * st["camera_samples"] and st["rays_any"] > 0 and px[..., :3].any()


def test_a_specular_bounce_that_escapes(gpu, monkeypatch):
    """a mirror mesh under the environment map: the reflected ray escapes with PS_SPECULAR set, so k_wf_accumulate reads the ray and adds
    the environment along it"""
    b = env_builder(gpu)
    b.material("mirror", Kr=(0.9, 0.8, 0.7))
    scenes._quad(b, (-6, -6, -1), (6, -6, -1), (6, 6, -1), (-6, 6, -1))
    b.material("matte", Kd=(0.7, 0.3, 0.3))
    scenes._quad(b, (-2, 3, -1), (2, 3, -1), (2, 3, 2), (-2, 3, 2))
    cam = PerspectiveCamera.look_at(gpu, (0.5, -7.0, 2.0), (0, 0, -0.5), (0, 0, 1), (64, 48), fov=45.0)
    (px,), st = on_off(monkeypatch, beauty(gpu, b.create_scene(), cam, (64, 48), PathIntegrator.new(5, 1.0), SMP))
    assert px[..., :3].any()


def null_quad(b, eye, at, half):
    """a square without material, facing the eye, centred at `at`"""
    n = np.asarray(eye, np.float64) - np.asarray(at, np.float64); n /= np.linalg.norm(n)
    u = np.cross(n, (0.0, 0.0, 1.0)); u /= np.linalg.norm(u)
    v = np.cross(n, u)
    c = np.asarray(at, np.float64)
    b.attribute_begin(); b.material("none")
    scenes._quad(b, *[tuple(float(x) for x in c + half * (su * u + sv * v)) for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1))])
    b.attribute_end()


def test_a_primitive_without_a_material_in_front_of_the_cubes(gpu, monkeypatch):
    """class 7 keeps its launch: the paths through the null square pass on without counting a bounce, so they are shaded one round later
    than the others and past round max_depth"""
    b, cam, res = scenes.instanced_cubes(gpu, n_copies=5, res=(96, 96), env_n=32)
    eye = np.array((1.9 * 26.0, -2.3 * 26.0, 1.4 * 26.0))
    null_quad(b, eye, 0.6 * eye, 9.0)
    sc = b.create_scene()
    for depth in (2, 5):
        (px,), st = on_off(monkeypatch, beauty(gpu, sc, cam, res, PathIntegrator.new(depth, 1.0), SMP))
        assert px[..., :3].any()


def test_rays_left_behind_the_last_round(gpu, monkeypatch):
    """Two large, nearly black planes facing each other behind a null square that fills the view.  A path bounces between the planes; at its
    fifth event (bounces = 4, one round late because of the null square: round 5 = max_depth) Russian roulette ends it with certainty
    (throughput 1e-15: q = 1 - beta rounds to 1) while its shadow and MIS rays are queued.  The poll then finds no active path but rays in
    the any-hit queue: late finish traces them behind the loop, the old route in a further round.  Same rays_any, same film."""
    b = env_builder(gpu)
    b.material("matte", Kd=(1e-3, 1e-3, 1e-3))
    scenes._quad(b, (-400, -400, -1), (400, -400, -1), (400, 400, -1), (-400, 400, -1))
    scenes._quad(b, (-400, -400, 1), (-400, 400, 1), (400, 400, 1), (400, -400, 1))
    eye, at = (0.0, -3.0, 0.0), (0.0, 0.0, -0.4)
    null_quad(b, eye, (0.0, -2.0, -0.13), 4.0)
    cam = PerspectiveCamera.look_at(gpu, eye, at, (0, 0, 1), (48, 40), fov=40.0)
    (px,), st = on_off(monkeypatch, beauty(gpu, b.create_scene(), cam, (48, 40), PathIntegrator.new(5, 1.0), SMP))
    assert st["rays_any"] > 0 and px[..., :3].any()


def test_the_hooks_read_the_final_radiance(gpu, monkeypatch, cubes):
    """a pass hook reads WfBuffers::rad: k_wf_accumulate stores the finished radiance there when one is installed.  Moments (film and
    moment planes) and a filtered film (radius 1.25), knob on against off"""
    sc, cam, res = cubes
    integ = PathIntegrator(5, 1.0)

    def moments():
        _, film, mom, st = M.render_moments(gpu, None, cam, res, integ, RandomSampler(13, 2, indexed=True), scene=sc)
        return (film.pixels, mom), st

    def filtered():
        _, film, st = FL.render_filtered(gpu, None, cam, res, integ, SMP, FL.Filter("gaussian", (1.25, 1.25), be=gpu), scene=sc)
        return (film.pixels,), st

    (px, mom), _ = on_off(monkeypatch, moments)
    assert px[..., :3].any() and mom.any()
    (fpx,), _ = on_off(monkeypatch, filtered)
    assert fpx[..., :3].any()


def test_a_scene_with_other_lights_keeps_the_old_route(gpu, monkeypatch):
    """the all-materials scene (point, distant and area lights): not an environment-only scene, so the knob changes nothing"""
    b, cam, res = _materials_scene(gpu)
    on_off(monkeypatch, beauty(gpu, b.create_scene(), cam, res, PathIntegrator.new(5, 1.0), RandomSampler(4, 5, indexed=True)))
