"""Loop subdivision on the GPU (include/fountain_hip_subdiv.h): the kernels against the host twin, which shares their per-element code
and is itself checked against a float64 restatement in tests/test_subdiv_cpu.py -- bit for bit, positions, normals and indices, on every
mesh and level of tests/_subdiv_common.py, into outputs pre-filled with sentinels; repeated calls, untouched inputs; and refined meshes
rendered on the GPU against the CPU oracle given the same refined mesh."""
import ctypes as C

import numpy as np
import pytest

from fountain_amd import PathIntegrator, PerspectiveCamera, RandomSampler, SceneBuilder, scenes, subdiv
from fountain_amd import _abi as A

import _subdiv_common as K

pytestmark = pytest.mark.gpu
F32 = np.float32
_twin = {}


def twin(gpu, name, level):
    if (name, level) not in _twin:
        P, idx = K.mesh(name)
        _twin[(name, level)] = subdiv.loop_subdivide_cpu(gpu, P, idx, level)
    return _twin[(name, level)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name,level", K.CASES, ids=K.CASE_IDS)
def test_device_equals_the_twin_bit_for_bit(gpu, name, level):
    P, idx = K.mesh(name)
    P0, idx0 = P.copy(), idx.copy()
    want = twin(gpu, name, level)
    lib = subdiv._lib(gpu)[1]
    nv, nf = want[0].shape[0], want[2].shape[0]
    # sentinels: a NaN pattern in the floats, an index no mesh has; one guard row behind each output
    out_P, out_N = np.full((nv + 1, 3), np.nan, F32), np.full((nv + 1, 3), np.nan, F32)
    out_idx = np.full((nf + 1, 3), 0xdeadbeef, np.uint32)
    rc = lib.ftn_loop_subdivide(P.ctypes.data, P.shape[0], idx.ctypes.data, idx.shape[0], level, out_P.ctypes.data, out_N.ctypes.data, out_idx.ctypes.data, -1)
    gpu.check(rc)
    assert np.array_equal(out_idx[:nf], want[2]) and (out_idx[nf] == 0xdeadbeef).all()
    assert np.array_equal(bits(out_P[:nv]), bits(want[0])) and np.isnan(out_P[nv]).all()
    assert np.array_equal(bits(out_N[:nv]), bits(want[1])) and np.isnan(out_N[nv]).all()
    assert np.array_equal(bits(P), bits(P0)) and np.array_equal(idx, idx0)


def test_repeated_calls_are_identical(gpu):
    for name, level in (("icosahedron", 3), ("grid25", 3)):
        P, idx = K.mesh(name)
        a = subdiv.loop_subdivide(gpu, P, idx, level)
        b = subdiv.loop_subdivide(gpu, P, idx, level)
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, twin(gpu, name, level)))


def test_degenerate_normals_are_refused_on_the_device_too(gpu):
    from fountain_amd import FountainError
    P, idx = K.mesh("octahedron")
    with pytest.raises(FountainError) as e:
        subdiv.loop_subdivide(gpu, np.zeros_like(P), idx, 2)
    assert e.value.code == A.FTN_ERR_INVALID_ARGUMENT and str(e.value).endswith("vertex 0")


def _octahedron_scene(be):
    """the level-3 octahedron, glossy, under a 32 x 32 environment map"""
    rng = np.random.default_rng(7)
    env = (0.2 + rng.random((32, 32, 3))).astype(F32)
    env[8:12, 20:24] *= 20.0
    b = SceneBuilder(be)
    b.light_source("infinite", texels=env)
    b.attribute_begin(); b.material("plastic", Kd=(0.3, 0.4, 0.6), Ks=(0.4, 0.4, 0.4), roughness=0.15); b.rotate(25, (0, 0, 1))
    P, idx = K.mesh("octahedron")
    b.shape("loopsubdiv", P=P, indices=idx, levels=3)
    b.attribute_end()
    return b, PerspectiveCamera.look_at(be, (2.2, -2.6, 1.6), (0, 0, 0), (0, 0, 1), (32, 32), fov=35.0)


def _grid_light_scene(be):
    """the bumped grid, refined twice, as an area light over a matte floor: it emits to the side of its faces' winding"""
    b = SceneBuilder(be)
    b.attribute_begin(); b.material("matte", Kd=(0.0, 0.0, 0.0)); b.area_light_source("diffuse", L=(6.0, 5.0, 4.0))
    b.translate((-1.5, -1.5, 2.0)); b.rotate(180, (1, 0, 0)); b.translate((0, -3, 0))
    P, idx = K.mesh("grid4")
    b.shape("loopsubdiv", P=P, indices=idx, levels=2)
    b.attribute_end()
    b.material("matte", Kd=(0.6, 0.6, 0.6))
    scenes._quad(b, (-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0))
    return b, PerspectiveCamera.look_at(be, (5, -6, 3.5), (0, 0, 1), (0, 0, 1), (32, 32), fov=40.0)


@pytest.mark.parametrize("pipeline", [A.FTN_PIPELINE_MEGAKERNEL, A.FTN_PIPELINE_WAVEFRONT])
@pytest.mark.parametrize("which", ["octahedron", "grid_light"])
def test_refined_meshes_render_like_the_oracle(gpu, orc_det, which, pipeline):
    """32 x 32, 4 spp: the builder refines on the GPU for the product and with the host twin for the oracle -- the same mesh -- and the
    films agree as every other scene's do (bit for bit but for the pixels that received a spill sample)"""
    make = _octahedron_scene if which == "octahedron" else _grid_light_scene
    films = []
    for be, kw in ((orc_det, {}), (gpu, dict(pipeline=pipeline))):
        b, cam = make(be)
        _, px, st, _ = scenes.render(be, b, cam, (32, 32), PathIntegrator(5, 1.0), RandomSampler(4, 0, indexed=True), backend_kwargs=kw)
        films.append((px, st))
    (ref, sto), (px, st) = films
    assert st["rays_closest"] == sto["rays_closest"] and st["rays_any"] == sto["rays_any"]
    diff = (bits(px) != bits(ref)).any(axis=-1)
    assert int(diff.sum()) <= 4 * st["spill_samples"] and np.allclose(px, ref, rtol=2e-6, atol=1e-7)
    assert np.isfinite(px).all() and px[..., :3].max() > 0
    if which == "grid_light":
        assert px[16:, :, :3].max() > 0.05                      # the floor is lit: the light faces it
