"""The previous-position pass on the GPU (include/fountain_hip_motion.h, fountain_amd/motion.py): a replay from the oracle's camera rays,
the current scene's ftn_intersect and ftn_intersect_full, and the PREVIOUS scene description's vertices and transforms (tests/_motion_ref.py), bit for bit,
on the smallest scenes that reach each branch; equal scenes against the G-buffer; film and call layout; the device resolve, motion
vectors and motion-aware accumulation against their host twins; the refusal of scenes that do not correspond; the command line."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from fountain_amd import Film, FountainError, PerspectiveCamera, RandomSampler, SceneBuilder, scenes, _abi as A
from fountain_amd import gbuffer as G
from fountain_amd import motion as M
from fountain_amd import temporal as T

import _gbuffer_ref as GR
import _motion_ref as MR

pytestmark = pytest.mark.gpu
F32 = np.float32
bits = GR.bits
SPP, SEED = 3, 77
q = scenes._quad


# ------------------------------------------------------------------ scenes: make(be, frame), frame 0 the previous one, 1 the current one
def _floor_and_light(b):
    b.light_source("point", I=(8, 8, 8), from_=(0, -3, 3))
    b.material("matte", Kd=(0.5, 0.5, 0.5))


def two_triangles(be, frame, res=(24, 16)):
    """two loose triangles whose bounding boxes share their centre, so that the builder cannot split them: one leaf, no four-box records;
    both deform between the frames"""
    b = SceneBuilder(be)
    _floor_and_light(b)
    d = 0.25 * frame
    b.shape("trianglemesh", P=[(-1 - d, 0, -0.5), (1 + d, 0, -0.5), (0, 0, 1)], indices=[0, 1, 2])
    b.shape("trianglemesh", P=[(-1, 0.5 + d, 1), (1, 0.5 + d, 1), (0, -0.5 - d, -0.5)], indices=[0, 1, 2])
    cam = PerspectiveCamera.look_at(be, (0, -4, 0.25), (0, 0, 0.25), (0, 0, 1), res, fov=40.0)
    return b, cam, res


def swapping_quads(be, frame, res=(24, 16)):
    """two quads that swap places along x, the axis the BVH splits on: the scenes' primitive orders differ"""
    b = SceneBuilder(be)
    _floor_and_light(b)
    for x in ((-1.0, 1.0) if frame else (1.0, -1.0)):
        q(b, (x - 0.6, 0, -0.6), (x + 0.6, 0, -0.6), (x + 0.6, 0.2, 0.6), (x - 0.6, 0.2, 0.6))
    cam = PerspectiveCamera.look_at(be, (0, -5, 0), (0, 0, 0), (0, 0, 1), res, fov=40.0)
    return b, cam, res


def cornell(be, frame, res=(40, 24)):
    """the Cornell fixture's walls and three spheres: one translated, one scaled through its transform, one left alone"""
    b = SceneBuilder(be)
    b.material("matte", Kd=(0.73, 0.73, 0.73))
    q(b, (-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1))
    q(b, (-1, -1, 1), (-1, 1, 1), (1, 1, 1), (1, -1, 1))
    q(b, (-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1))
    b.material("matte", Kd=(0.65, 0.05, 0.05))
    q(b, (-1, -1, -1), (-1, 1, -1), (-1, 1, 1), (-1, -1, 1))
    b.material("matte", Kd=(0.12, 0.45, 0.15))
    q(b, (1, -1, -1), (1, -1, 1), (1, 1, 1), (1, 1, -1))
    b.attribute_begin()
    b.material("matte", Kd=(0, 0, 0))
    b.area_light_source("diffuse", L=(15.0, 15.0, 15.0))
    q(b, (-0.25, -0.25, 0.995), (-0.25, 0.25, 0.995), (0.25, 0.25, 0.995), (0.25, -0.25, 0.995))
    b.attribute_end()
    b.attribute_begin()
    b.material("matte", Kd=(0.6, 0.6, 0.3))
    b.translate((-0.45 + 0.1 * frame, 0.3, -0.65 + 0.05 * frame))
    b.shape("sphere", radius=0.35)
    b.attribute_end()
    b.attribute_begin()
    b.material("mirror", Kr=(0.9, 0.9, 0.9))
    b.translate((0.45, 0.1, -0.6))
    if frame:
        b.scale(1.0, 0.8, 1.2)
    b.shape("sphere", radius=0.4)
    b.attribute_end()
    b.attribute_begin()
    b.material("plastic", Kd=(0.2, 0.3, 0.6), Ks=(0.3, 0.3, 0.3), roughness=0.1)
    b.translate((0.0, -0.45, -0.8))
    b.shape("sphere", radius=0.2)
    b.attribute_end()
    cam = PerspectiveCamera.look_at(be, (0, -3.4, 0), (0, 0, 0), (0, 0, 1), res, fov=40.0)
    return b, cam, res


def subdivided(be, frame, res=(24, 16)):
    """an octahedron refined twice (128 triangles with limit normals) whose control points move, over a floor"""
    b = SceneBuilder(be)
    _floor_and_light(b)
    q(b, (-3, -3, -1.2), (3, -3, -1.2), (3, 3, -1.2), (-3, 3, -1.2))
    s = 0.2 * frame
    P = [(1 + s, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1 - s, 0), (0, 0, 1 + s), (0, 0, -1)]
    idx = [0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5]
    b.material("matte", Kd=(0.7, 0.4, 0.3))
    b.shape("loopsubdiv", P=P, indices=idx, levels=2)
    cam = PerspectiveCamera.look_at(be, (0.5, -4, 1.0), (0, 0, 0), (0, 0, 1), res, fov=40.0)
    return b, cam, res


def shell(be, frame, res=(24, 16)):
    """a block that moves on a floor behind a null-material quad: every camera ray that reaches it passed through first"""
    b = SceneBuilder(be)
    b.light_source("infinite", L=(0.5, 0.5, 0.5))
    b.material("matte", Kd=(0.6, 0.6, 0.6))
    q(b, (-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0))
    x = 0.3 * frame
    b.material("matte", Kd=(0.7, 0.3, 0.2))
    q(b, (x - 0.5, -0.5, 0.8), (x + 0.5, -0.5, 0.8), (x + 0.5, 0.5, 0.8), (x - 0.5, 0.5, 0.8))
    q(b, (x - 0.5, -0.5, 0.0), (x + 0.5, -0.5, 0.0), (x + 0.5, -0.5, 0.8), (x - 0.5, -0.5, 0.8))
    b.material("none")
    q(b, (-1.5, -1.5, 0.0), (1.5, -1.5, 0.0), (1.5, -1.5, 2.0), (-1.5, -1.5, 2.0))
    cam = PerspectiveCamera.look_at(be, (0.3, -5.0, 2.2), (0.0, 0.0, 0.5), (0, 0, 1), res, fov=40.0)
    return b, cam, res


SCENES = dict(two_triangles=two_triangles, swapping_quads=swapping_quads, cornell=cornell, subdivided=subdivided, shell=shell)


@functools.lru_cache(maxsize=None)
def _replay(gpu, orc, name, same=False, crop=(0.0, 0.0, 1.0, 1.0), tiles=None, res=None):
    make = SCENES[name] if res is None else (lambda be, frame: SCENES[name](be, frame, res))
    return MR.replay(gpu, orc, make, SPP, SEED, crop=crop, tiles=tiles, same=same)


def _pair(gpu, name, res=None):
    kw = {} if res is None else dict(res=res)
    b0, _, _ = SCENES[name](gpu, 0, **kw)
    b1, cam, res = SCENES[name](gpu, 1, **kw)
    return b1.create_scene(), b0.create_scene(), cam, res


def _smp(first=0, count=0):
    return RandomSampler(SPP, SEED, indexed=True, first_sample=first, sample_count=count)


# ------------------------------------------------------------------ 1. the replay
@pytest.mark.parametrize("name", sorted(SCENES))
def test_replay(gpu, orc_det, name):
    """every camera sample's p' and ns' restated from the previous scene description, summed on the film rule: bit-equal"""
    ref = _replay(gpu, orc_det, name)
    scene, prev, cam, res = _pair(gpu, name)
    mv8, raw, st = M.render_motion(gpu, None, cam, res, _smp(), scene=scene, prev_scene=prev)
    print("%s: %d samples, %d surfaces, %d rays, kinds %r" % (name, ref["n"], ref["hits"], ref["rays_closest"], sorted(ref["kinds"])))
    assert (st["camera_samples"], st["rays_closest"], st["spill_samples"]) == (ref["n"], ref["rays_closest"], ref["n_spill"])
    MR.assert_replayed(raw, ref, name)
    _, gb_raw, gst = G.render_gbuffer(gpu, None, cam, res, _smp(), scene=scene)
    assert np.array_equal(bits(raw[..., 6:8]), bits(gb_raw[..., 10:12])) and st["rays_closest"] == gst["rays_closest"]
    assert np.array_equal(bits(mv8), bits(M.motion_resolve(gpu, raw)))
    # the scene reaches the branch it is here for
    assert 0 < ref["hits"] and (0, True) in ref["kinds"] or name == "cornell"
    if name == "cornell":
        assert {(1, True), (1, False), (0, False)} <= ref["kinds"]          # a moved sphere, one that stands, the walls
    if name == "swapping_quads":
        assert not np.array_equal(scene.nodes()[1], prev.nodes()[1]), "the two scenes' primitive orders agree: the remap is not exercised"
    if name == "two_triangles":
        assert len(scene.nodes()[0]) == 1
    if name == "shell":
        assert ref["rays_closest"] > ref["n"], "no camera ray passed through the shell"
    if name == "subdivided":
        assert scene.info()["n_prims"] == 130 <= 640


def test_replay_with_a_wide_filter(gpu, orc_det):
    """cornell under a box filter of radius (0.75, 0.5): half the samples reach a neighbour in x, so the spill sums and their merge carry
    a large part of the film; pixels no foreign sample reached stay bit-equal, the others within the reordering bound"""
    radius = (0.75, 0.5)
    ref = MR.replay(gpu, orc_det, SCENES["cornell"], SPP, SEED, radius=radius)
    scene, prev, cam, res = _pair(gpu, "cornell")
    _, raw, st = M.render_motion(gpu, None, cam, res, _smp(), scene=scene, prev_scene=prev, film=GR.film(gpu, res, (0.0, 0.0, 1.0, 1.0), radius))
    print("radius %r: %d samples, %d spilled, %.3f of the pixels with a foreign sample" % (radius, ref["n"], ref["n_spill"], ref["foreign"].mean()))
    assert (st["camera_samples"], st["rays_closest"], st["spill_samples"]) == (ref["n"], ref["rays_closest"], ref["n_spill"])
    MR.assert_replayed(raw, ref, "cornell, radius %r" % (radius,))
    assert 0.05 < ref["foreign"].mean() < 0.95, "one of the two pixel classes is all but empty"


@pytest.mark.parametrize("name", sorted(SCENES))
def test_equal_scenes_give_the_gbuffer(gpu, name):
    """a previous scene built like the current one (another scene object): the position and normal sums are the G-buffer's bit for bit,
    and so are the weights"""
    b1, cam, res = SCENES[name](gpu, 1)
    b2, _, _ = SCENES[name](gpu, 1)
    scene, twin = b1.create_scene(), b2.create_scene()
    _, raw, _ = M.render_motion(gpu, None, cam, res, _smp(), scene=scene, prev_scene=twin)
    _, gb, _ = G.render_gbuffer(gpu, None, cam, res, _smp(), scene=scene)
    own = gb[..., 11] == SPP                                       # (pixels without a sample of another pixel: the spill sums' order is free)
    assert own.mean() > 0.95
    assert np.array_equal(bits(raw[..., 6:8]), bits(gb[..., 10:12]))
    assert np.array_equal(bits(raw[own][:, 0:3]), bits(gb[own][:, 6:9])) and np.array_equal(bits(raw[own][:, 3:6]), bits(gb[own][:, 3:6]))
    assert np.allclose(raw[..., 0:3], gb[..., 6:9], rtol=2e-6, atol=1e-6) and np.allclose(raw[..., 3:6], gb[..., 3:6], rtol=2e-6, atol=1e-6)
    _, same, _ = M.render_motion(gpu, None, cam, res, _smp(), scene=scene, prev_scene=scene)       # the scene against itself
    assert np.array_equal(bits(same[own]), bits(raw[own])) and np.array_equal(bits(same[..., 6:8]), bits(raw[..., 6:8]))


# ------------------------------------------------------------------ 2. film and call layout
def test_film_and_call_layout(gpu, orc_det, monkeypatch):
    """a 33 x 17 film with an unaligned crop: the sample range split over two calls, strided tile ranges composed, several passes forced
    (FTN_WF_PATHS_M, as tests/test_gbuffer.py forces them; 0 gives passes of one sample) and the torch entry: the weights identical, the
    float sums as the film rule orders them"""
    import torch
    name, res, crop = "cornell", (33, 17), (0.1, 0.15, 0.95, 0.9)
    scene, prev, cam, _ = _pair(gpu, name, res)
    ref = _replay(gpu, orc_det, name, crop=crop, res=res)
    own = ~ref["foreign"]
    _, one, st1 = M.render_motion(gpu, None, cam, res, _smp(), scene=scene, prev_scene=prev, crop=crop)
    assert one.shape[:2] != (17, 33) and one.shape == ref["acc"].shape
    MR.assert_replayed(one, ref, "one call")

    def same(got, what):
        assert np.array_equal(bits(got[..., 6:8]), bits(one[..., 6:8])), what
        assert np.array_equal(bits(got[own]), bits(one[own])), what
        assert np.allclose(got, one, rtol=2e-6, atol=1e-6), what

    _, two, sa = M.render_motion(gpu, None, cam, res, _smp(0, 1), scene=scene, prev_scene=prev, crop=crop)
    _, _, sb = M.render_motion(gpu, None, cam, res, _smp(1, SPP - 1), scene=scene, prev_scene=prev, crop=crop, raw=two)
    same(two, "a sample range over two calls")
    assert sa["camera_samples"] + sb["camera_samples"] == st1["camera_samples"] == ref["n"]
    _, tl, _ = M.render_motion(gpu, None, cam, res, _smp(), scene=scene, prev_scene=prev, crop=crop, tiles=(0, 2, 0))
    M.render_motion(gpu, None, cam, res, _smp(), scene=scene, prev_scene=prev, crop=crop, tiles=(1, 2, 0), raw=tl)
    same(tl, "strided tile ranges composed")
    reft = _replay(gpu, orc_det, name, crop=crop, tiles=(1, 2, 0), res=res)
    _, odd, _ = M.render_motion(gpu, None, cam, res, _smp(), scene=scene, prev_scene=prev, crop=crop, tiles=(1, 2, 0))
    MR.assert_replayed(odd, reft, "every second tile")
    monkeypatch.setenv("FTN_WF_PATHS_M", "0")
    _, passes, stp = M.render_motion(gpu, None, cam, res, _smp(), scene=scene, prev_scene=prev, crop=crop)
    monkeypatch.delenv("FTN_WF_PATHS_M")
    assert np.array_equal(bits(passes), bits(one)) and stp["camera_samples"] == st1["camera_samples"] and stp["rays_closest"] == st1["rays_closest"]
    # the torch entry, the device resolve
    film = Film(gpu, res, crop)
    t = torch.zeros((film.height, film.width, 8), dtype=torch.float32, device="cuda:0")
    M.render_motion_torch(scene, prev, cam, film, _smp(), t)
    torch.cuda.synchronize()
    same(t.cpu().numpy(), "the torch entry")
    out = torch.empty_like(t)
    M.motion_resolve_torch(gpu, t, out)
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(M.motion_resolve(gpu, t.cpu().numpy())))


# ------------------------------------------------------------------ 3. the device stages against their host twins
def test_device_stages_equal_their_twins(gpu):
    """resolve, motion vectors and the motion-aware accumulation on rendered buffers of two frames under a camera that moves too: the
    device paths, host-buffer and torch, equal the host twins bit for bit"""
    import torch
    scene, prev, cam, res = _pair(gpu, "cornell")
    pcam = PerspectiveCamera.look_at(gpu, (0.15, -3.4, 0.05), (0, 0, 0), (0, 0, 1), res, fov=40.0)
    film = Film(gpu, res)
    gbs = []
    for sc, c in ((prev, pcam), (scene, cam)):
        r, _, _ = G.render_gbuffer(gpu, None, c, res, _smp(), scene=sc)
        gbs.append(np.ascontiguousarray(np.concatenate([r[k] for k in G.CHANNELS], axis=-1)))
    mv8, raw, _ = M.render_motion(gpu, None, cam, res, _smp(), scene=scene, prev_scene=prev)
    rng = np.random.default_rng(3)
    h, w = mv8.shape[:2]
    frames = [(rng.uniform(0.1, 1.0, (h, w, 3)).astype(F32), gb, rng.uniform(0.0, 0.01, (h, w, 4)).astype(F32)) for gb in gbs]
    mv8 = mv8.copy()
    (ya, xa), (yb, xb) = (h // 2, w // 2), (h // 2 - 2, w // 2 + 3)  # two pixels of the back wall
    assert gbs[1][ya, xa, 10] > 0 and gbs[1][yb, xb, 10] > 0
    mv8[ya, xa, 0], mv8[yb, xb, 6] = np.nan, 0.0                     # an edge row each: a NaN position, the other coverage class
    for cams in ((pcam, cam), (cam, cam)):                           # a moving camera, and equal cameras
        hist0 = T.temporal_accumulate_cpu(gpu, *frames[0], cams[0], film)[0]
        prv = (cams[0], frames[0][1], hist0)
        want = T.temporal_accumulate_cpu(gpu, *frames[1], cams[1], film, prv, motion=mv8)
        got = T.temporal_accumulate(gpu, *frames[1], cams[1], film, prv, motion=mv8)
        for g, x in zip(got, want):
            assert np.array_equal(bits(g), bits(x))
        static = T.temporal_accumulate_cpu(gpu, *frames[1], cams[1], film, prv)
        assert (bits(static[0]) != bits(want[0])).any(), "mv8 changed nothing: the spheres moved"
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        outs = [torch.empty((h, w, k), dtype=torch.float32, device="cuda:0") for k in (8, 3, 4)]
        T.temporal_accumulate_torch(gpu, *(dev(a) for a in frames[1]), cams[1], film, *outs, prev=(cams[0], dev(prv[1]), dev(prv[2])), motion=dev(mv8))
        torch.cuda.synchronize()
        for g, x in zip(outs, want):
            assert np.array_equal(bits(g.cpu().numpy()), bits(x))
        mo_cpu = M.motion_vectors_cpu(gpu, mv8, frames[1][1], cams[1], cams[0], film)
        assert np.array_equal(bits(M.motion_vectors(gpu, mv8, frames[1][1], cams[1], cams[0], film)), bits(mo_cpu))
        mo = torch.empty((h, w, 2), dtype=torch.float32, device="cuda:0")
        M.motion_vectors_torch(gpu, dev(mv8), dev(frames[1][1]), cams[1], cams[0], film, mo)
        torch.cuda.synchronize()
        assert np.array_equal(bits(mo.cpu().numpy()), bits(mo_cpu))
        assert np.isnan(mo_cpu[ya, xa]).all() and np.isnan(mo_cpu[yb, xb]).all() and np.isfinite(mo_cpu).mean() > 0.9
    # under equal cameras only what moved has a motion
    moved = (bits(mv8[..., :3]) != bits(frames[1][1][..., 6:9])).any(-1)
    fin = np.isfinite(mo_cpu).all(-1)
    assert (mo_cpu[fin & ~moved] == 0).all() and (np.abs(mo_cpu[fin & moved]).max(-1) > 0).mean() > 0.9


# ------------------------------------------------------------------ 4. refusals
def test_scenes_that_do_not_correspond_are_refused(gpu):
    """another count, another kind in the same place, a changed sphere radius: FTN_ERR_INVALID_ARGUMENT naming the primitive, before the
    sampler and pipeline refusals, nothing rendered into the caller's buffer"""
    def build(extra=None, radius=0.3, first_sphere=True):
        b = SceneBuilder(gpu)
        _floor_and_light(b)
        q(b, (-2, 1, -1), (2, 1, -1), (2, 1, 1), (-2, 1, 1))
        if first_sphere:
            b.shape("sphere", radius=radius)
        else:
            b.shape("trianglemesh", P=[(0, 0, 0), (1, 0, 0), (0, 0, 1)], indices=[0, 1, 2])
        if extra:
            b.shape("trianglemesh", P=[(0, 0, 0), (-1, 0, 0), (0, 0, 1)], indices=[0, 1, 2])
        return b.create_scene()
    res = (16, 16)
    cam = PerspectiveCamera.look_at(gpu, (0, -4, 0), (0, 0, 0), (0, 0, 1), res, fov=40.0)
    base = build()
    raw = np.full((16, 16, 8), 7.0, F32)
    for other, word in ((build(extra=True), "primitive 3 has no counterpart"), (build(first_sphere=False), "primitive 2 is a sphere here and a triangle"),
                        (build(radius=0.31), "primitive 2, a sphere")):
        for smp in (_smp(), RandomSampler(SPP, SEED, indexed=False)):          # the scenes come before the sampler
            with pytest.raises(FountainError) as e:
                M.render_motion(gpu, None, cam, res, smp, scene=base, prev_scene=other, raw=raw)
            assert e.value.code == A.FTN_ERR_INVALID_ARGUMENT and word in str(e.value), str(e.value)
    assert (raw == 7.0).all()
    with pytest.raises(FountainError) as e:
        M.render_motion(gpu, None, cam, res, RandomSampler(SPP, SEED, indexed=False), scene=base, prev_scene=build(), raw=raw)
    assert e.value.code == A.FTN_ERR_UNSUPPORTED and "FTN_SAMPLER_INDEXED" in str(e.value)
    with pytest.raises(FountainError) as e:
        M.render_motion(gpu, None, cam, res, _smp(), scene=base, prev_scene=build(), raw=raw, pipeline=A.FTN_PIPELINE_MEGAKERNEL)
    assert e.value.code == A.FTN_ERR_UNSUPPORTED and (raw == 7.0).all()
    _, ok, _ = M.render_motion(gpu, None, cam, res, _smp(), scene=base, prev_scene=build())
    assert ok[..., 7].min() >= SPP


# ------------------------------------------------------------------ 5. the command line
FRAME = """Film "image" "integer xresolution" [ 24 ] "integer yresolution" [ 16 ] "string filename" [ "f.exr" ]
Sampler "random" "integer pixelsamples" [ 4 ]
LookAt %g -4 0  0 0 0  0 0 1
Camera "perspective" "float fov" [ 40 ]
WorldBegin
LightSource "point" "point from" [0 -3 2] "rgb I" [10 10 10]
Material "matte" "rgb Kd" [.5 .5 .5]
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-2 1 -1  2 1 -1  2 1 1  -2 1 1]
AttributeBegin
Translate %g 0 0
Shape "sphere" "float radius" 0.4
AttributeEnd
WorldEnd
"""
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "temporal_cli_static.json")


def test_cli_dynamic(gpu, tmp_path):
    """two frames, the sphere and the camera moved: the expected files, out_1_motion.exr equal to motion_vectors of the same renders, and
    without --dynamic the bytes this command wrote before it knew the flag (tests/golden/temporal_cli_static.json: their SHA-256)"""
    import hashlib
    import json
    from fountain_amd import PbrtScene, read_exr
    files = []
    for k, (eye, x) in enumerate(((0.0, -0.3), (0.2, 0.3))):
        files.append(tmp_path / ("f%d.pbrt" % k))
        files[-1].write_text(FRAME % (eye, x))
    out = tmp_path / "dyn" / "o.exr"
    os.makedirs(out.parent)
    assert T.main([str(f) for f in files] + ["-o", str(out), "--samples", "4", "--dynamic"]) == 0
    assert sorted(os.listdir(out.parent)) == ["o_0.exr", "o_0_accumulated.exr", "o_1.exr", "o_1_accumulated.exr", "o_1_motion.exr"]
    fr = [PbrtScene(str(f), gpu) for f in files]
    sc = [f.create_scene() for f in fr]
    smp = RandomSampler.new_with_seed(4, 1, indexed=True)
    mv8, _, _ = M.render_motion(gpu, None, fr[1].camera, None, smp, scene=sc[1], prev_scene=sc[0], film=fr[1].film())
    r, _, _ = G.render_gbuffer(gpu, None, fr[1].camera, None, smp, scene=sc[1], film=fr[1].film())
    gb12 = np.concatenate([r[c] for c in G.CHANNELS], axis=-1)
    want = M.motion_vectors(gpu, mv8, gb12, fr[1].camera, fr[0].camera, fr[1].film())
    got = read_exr(str(out.parent / "o_1_motion.exr"), gpu)
    assert np.array_equal(bits(got[..., :2]), bits(want)) and (got[..., 2] == 0).all()
    assert np.abs(want[np.isfinite(want).all(-1)]).max() > 1.0               # the sphere moved by several pixels
    # the dynamic frame differs from the static one where the sphere is
    static = tmp_path / "static" / "o.exr"
    os.makedirs(static.parent)
    assert T.main([str(f) for f in files] + ["-o", str(static), "--samples", "4"]) == 0
    assert sorted(os.listdir(static.parent)) == ["o_0.exr", "o_0_accumulated.exr", "o_1.exr", "o_1_accumulated.exr"]
    sha = {n: hashlib.sha256(open(static.parent / n, "rb").read()).hexdigest() for n in sorted(os.listdir(static.parent))}
    print("static run: %s" % json.dumps(sha))
    assert sha == json.load(open(GOLDEN))["sha256"]
    a, b = read_exr(str(static.parent / "o_1_accumulated.exr"), gpu), read_exr(str(out.parent / "o_1_accumulated.exr"), gpu)
    assert (bits(a) != bits(b)).any()
