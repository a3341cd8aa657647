"""The configurations, comparisons and properties of the integrator tests, shared by test_integrator_cpu.py (both oracle builds) and
test_integrator.py (the device, through the megakernel and through the wavefront pipeline with its counting and its production kernels).

Layer 1: tests/_integrator_ref.py against a library's radiance of every camera sample.  Layer 2: properties no reading of the reference enters.
Layer 3: the device against the deterministic oracle, sample by sample and bit for bit.

One camera sample is observed without a hook: on the oracle through orc_render_sample_log, on any library through a one-sample range of the indexed
sampler on a box film of radius 0.5, after which a pixel's sums hold rgb_to_xyz(0 + L) of exactly one sample."""
import functools

import numpy as np

from fountain_amd import (DirectLightingIntegrator, FountainError, PathIntegrator, PerspectiveCamera, RandomSampler, SamplerIntegrator, SceneBuilder,
                          WhittedIntegrator, _abi as A, scenes)

import _bsdf_ref as B
import _gbuffer_ref as GR
import _integrator_ref as IG
import _interaction_ref as IR
import _moments_ref as MR

F32 = np.float32
MAX_FRAGILE_SHARE = 0.02                              # per configuration; a condition on the configurations, not a measurement
MEGA, WAVE = A.FTN_PIPELINE_MEGAKERNEL, A.FTN_PIPELINE_WAVEFRONT
SETTINGS = {"megakernel": dict(pipeline=MEGA, count_traffic=True), "wavefront_counting": dict(pipeline=WAVE, count_traffic=True),
            "wavefront_production": dict(pipeline=WAVE, count_traffic=False)}
quad = scenes._quad


# ------------------------------------------------------------------ scenes
def cube(b, c, h):
    """an axis-aligned box of half-widths h around c, six quads"""
    (x0, y0, z0), (x1, y1, z1) = np.subtract(c, h), np.add(c, h)
    quad(b, (x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)); quad(b, (x0, y0, z1), (x0, y1, z1), (x1, y1, z1), (x1, y0, z1))
    quad(b, (x0, y0, z0), (x0, y0, z1), (x1, y0, z1), (x1, y0, z0)); quad(b, (x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1))
    quad(b, (x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (x0, y0, z1)); quad(b, (x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0))


def triangle_light(b, z=0.9, L=(12.0, 11.0, 9.0), half=0.45, at=(0.05, 0.1)):
    """one emitting triangle facing -z (a single emitter: the order of Scene::lights does not depend on the BVH)"""
    b.attribute_begin()
    b.material("matte", Kd=(0.0, 0.0, 0.0))
    b.area_light_source("diffuse", L=L)
    x, y = at
    b.shape("trianglemesh", P=[(x - half, y - half, z), (x - half, y + half, z), (x + half, y + half, z)], indices=[0, 1, 2])
    b.attribute_end()


def closed_box(be, res=16, albedo=1.0, light=True, sheet=False, fov=62.0, look=(0.0, 1.0, 0.5)):
    """a closed matte box [-1, 1]^3 with walls of different colours, the camera inside it, a triangle light under the ceiling; `sheet`: a quad
    without a material between the camera and the far wall"""
    b = SceneBuilder(be)
    a = albedo
    for kd, q in (((0.7, 0.7, 0.7), ((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1))), ((0.6, 0.65, 0.7), ((-1, -1, 1), (-1, 1, 1), (1, 1, 1), (1, -1, 1))),
                  ((0.7, 0.6, 0.5), ((-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1))), ((0.5, 0.5, 0.6), ((-1, -1, -1), (-1, -1, 1), (1, -1, 1), (1, -1, -1))),
                  ((0.65, 0.1, 0.1), ((-1, -1, -1), (-1, 1, -1), (-1, 1, 1), (-1, -1, 1))), ((0.15, 0.45, 0.2), ((1, -1, -1), (1, -1, 1), (1, 1, 1), (1, 1, -1)))):
        b.material("matte", Kd=tuple(a * k for k in kd))
        quad(b, *q)
    if light:
        triangle_light(b)
    if sheet:
        b.material("none")
        quad(b, (-0.7, -0.2, -0.6), (0.6, -0.2, -0.6), (0.6, -0.1, 0.7), (-0.7, -0.1, 0.7))
    cam = PerspectiveCamera.look_at(be, (0.03, -0.93, 0.07), look, (0, 0, 1), (res, res), fov=fov)
    return b, cam, (res, res)


def dented_box(be, res=16):
    """the closed box with a raised 2 x 2-cell platform whose vertex normals lean up to 25 degrees off the faces': the shading normal differs from the
    geometric one (abs_dot takes the shading normal, integrator/mod.rs:326, :348, path.rs:71, whitted.rs:54)"""
    b, cam, _ = closed_box(be, res, look=(0.0, 0.6, -0.6))          # the camera looks down at the platform
    g = np.linspace(-0.7, 0.7, 3)
    P = [(x, y + 0.2, -0.55) for y in g for x in g]
    lean = [(0.4, 0.2), (-0.3, 0.35), (0.1, -0.45), (-0.4, -0.1), (0.0, 0.0), (0.45, 0.3), (0.25, -0.3), (-0.2, 0.4), (-0.35, -0.35)]
    N = [(u, v, 1.0) / np.sqrt(u * u + v * v + 1.0) for u, v in lean]
    idx = []
    for j in range(2):
        for i in range(2):
            a = 3 * j + i
            idx += [a, a + 1, a + 4, a, a + 4, a + 3]
    b.material("plastic", Kd=(0.5, 0.45, 0.3), Ks=(0.3, 0.3, 0.3), roughness=0.2)
    b.shape("trianglemesh", P=P, N=N, indices=idx)
    return b, cam, (res, res)


def env_texels(w, h, seed):
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.2, 1.5, (h, w, 3))
    t[h // 3, w // 2] *= 6.0                          # one bright texel: the distribution is far from uniform
    return t.astype(F32)


def env_boxes(be, w, h, area, res=(20, 16)):
    """three boxes on a ground quad under a w x h environment map, alone or beside a triangle light"""
    b = SceneBuilder(be)
    b.attribute_begin(); b.rotate(25.0, (0.1, 0.2, 1.0)); b.light_source("infinite", texels=env_texels(w, h, 5 + w)); b.attribute_end()
    b.material("matte", Kd=(0.55, 0.5, 0.45))
    quad(b, (-6, -6, 0), (6, -6, 0), (6, 6, 0), (-6, 6, 0))
    for i, (c, hh, kd) in enumerate((((-1.1, 0.3, 0.5), (0.5, 0.5, 0.5), (0.7, 0.3, 0.2)), ((0.4, 0.9, 0.8), (0.45, 0.35, 0.8), (0.3, 0.6, 0.3)), ((1.2, -0.5, 0.3), (0.3, 0.4, 0.3), (0.3, 0.3, 0.7)))):
        b.material("matte", Kd=kd, sigma=20.0 * i)
        cube(b, c, hh)
    if area:
        triangle_light(b, z=2.6, L=(6.0, 6.0, 5.0), half=0.6)
    cam = PerspectiveCamera.look_at(be, (0.6, -5.2, 2.3), (0.1, 0.2, 0.45), (0, 0, 1), res, fov=38.0)
    return b, cam, res


def sphere_lamp(be, res=(20, 16)):
    """an emitting partial sphere (the whole sphere is sampled, sphere.rs:202-218) above three matte spheres"""
    b = SceneBuilder(be)
    b.attribute_begin(); b.material("matte", Kd=(0, 0, 0)); b.area_light_source("diffuse", L=(9, 8, 7)); b.translate((0.1, 0.0, 2.4))
    b.shape("sphere", radius=0.5, zmin=-0.5, zmax=0.25); b.attribute_end()
    for i, (c, r, kd) in enumerate((((-1.0, 0.2, 0.0), 0.6, (0.7, 0.4, 0.3)), ((0.3, -0.2, -0.1), 0.5, (0.4, 0.7, 0.4)), ((1.3, 0.5, 0.1), 0.55, (0.4, 0.4, 0.8)))):
        b.attribute_begin(); b.material("matte", Kd=kd, sigma=15.0 * i); b.translate(c); b.shape("sphere", radius=r); b.attribute_end()
    cam = PerspectiveCamera.look_at(be, (0.2, -4.5, 1.6), (0.15, 0.0, 0.5), (0, 0, 1), res, fov=40.0)
    return b, cam, res


def mirror_corridor(be, res=(16, 16)):
    """two facing mirrors, a matte floor and a triangle light the camera sees only through the mirrors"""
    b = SceneBuilder(be)
    b.material("mirror", Kr=(0.9, 0.85, 0.8))
    quad(b, (-1, -3, -1), (-1, 3, -1), (-1, 3, 1.5), (-1, -3, 1.5))
    quad(b, (1, -3, -1), (1, -3, 1.5), (1, 3, 1.5), (1, 3, -1))
    b.material("matte", Kd=(0.6, 0.6, 0.55))
    quad(b, (-1, -3, -1), (1, -3, -1), (1, 3, -1), (-1, 3, -1))
    triangle_light(b, z=1.4, L=(10.0, 10.0, 9.0), half=0.5, at=(0.0, -2.2))
    cam = PerspectiveCamera.look_at(be, (0.55, -1.7, 0.1), (-1.0, -0.6, 0.25), (0, 0, 1), res, fov=50.0)
    return b, cam, res


def textured_room(be, image, res=(20, 16)):
    """a floor with uvs under a checkerboard or an image map, a mirror ball (the direct-lighting integrator reaches the floor through a specular
    bounce as well, with that bounce's differentials; the path integrator hands the camera's on), a point light and a triangle light"""
    b = SceneBuilder(be)
    if image:
        rng = np.random.default_rng(23)
        img = rng.uniform(0.15, 0.9, (32, 16, 3)).astype(F32)
        b.texture("floor", "spectrum", "imagemap", texels=img, uscale=3.0, vscale=2.0)
    else:
        b.texture("floor", "spectrum", "checkerboard", uscale=5.0, vscale=7.0, tex1=(0.75, 0.7, 0.6), tex2=(0.2, 0.25, 0.4))
    b.light_source("point", I=(14, 14, 14), from_=(-1.2, -0.8, 2.2))
    b.material("matte", Kd="floor")
    b.shape("trianglemesh", P=[(-4, -3, 0), (4, -3, 0), (4, 7, 0), (-4, 7, 0)], uv=[(0.013, 0.021), (1.013, 0.021), (1.013, 1.021), (0.013, 1.021)], indices=[0, 1, 2, 0, 2, 3])
    b.attribute_begin(); b.material("mirror"); b.translate((0.5, 1.4, 0.7)); b.shape("sphere", radius=0.7); b.attribute_end()
    triangle_light(b, z=3.0, L=(7.0, 7.0, 6.0), half=0.7, at=(0.3, 1.0))
    cam = PerspectiveCamera.look_at(be, (0.0, -3.2, 1.3), (0.15, 1.0, 0.35), (0, 0, 1), res, fov=48.0)
    return b, cam, res


def materials_small(be):
    from test_gpu_parity import _materials_scene
    b, _, _ = _materials_scene(be)
    res = (24, 16)                                    # a wider view than the parity tests': fewer of the samples meet the rotated spheres (see "gallery")
    cam = PerspectiveCamera.look_at(be, (0, -7, 2.5), (0, 0, -0.3), (0, 0, 1), res, fov=62.0, lens_radius=0.08, focal_dist=7.3)
    return b, cam, res


def gallery(be, res=(24, 16)):
    """Oren-Nayar, anisotropic metal, plastic, rough glass, mirror and an isotropic metal on translated spheres over a matte floor; a point, a
    distant and an area light (one triangle); a thin lens"""
    b = SceneBuilder(be)
    b.light_source("point", I=(40, 40, 40), from_=(0, -2, 3))
    b.light_source("distant", L=(1.5, 1.4, 1.2), from_=(1, -1, 2), to=(0, 0, 0))
    b.material("matte", Kd=(0.6, 0.6, 0.6), sigma=25.0)
    quad(b, (-6, -6, -1), (6, -6, -1), (6, 6, -1), (-6, 6, -1))
    triangle_light(b, z=3.5, L=(8.0, 8.0, 8.0), half=0.8, at=(0.2, 0.3))
    specs = [("metal", dict(eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14), uroughness=0.02, vroughness=0.2)), ("plastic", dict(Kd=(0.3, 0.1, 0.1), Ks=(0.4, 0.4, 0.4), roughness=0.05)),
             ("glass", dict(uroughness=0.1, vroughness=0.1, eta=1.5)), ("mirror", dict()), ("metal", dict(eta=(1.5, 1.0, 0.5), k=(3, 2.5, 2), roughness=0.3, remaproughness=False))]
    for i, (m, kw) in enumerate(specs):
        b.attribute_begin(); b.material(m, **kw); b.translate((-2.4 + 1.2 * i, 0.2 * i, -0.45)); b.shape("sphere", radius=0.55); b.attribute_end()
    cam = PerspectiveCamera.look_at(be, (0, -7, 2.5), (0, 0, -0.3), (0, 0, 1), res, fov=42.0, lens_radius=0.08, focal_dist=7.3)
    return b, cam, res


def emitters(be, res=(16, 16)):
    """five emitting triangles and an emitting sphere spread over space above a matte floor and in front of a matte wall, and a point light: the order
    of Scene::lights for several emitters is the BVH's primitive order (scene/mod.rs:38-42), which differs from the order they are stated in; the
    traversal tests check that order from the tree, so that area_order is a checked fact here"""
    b = SceneBuilder(be)
    b.light_source("point", I=(6, 6, 6), from_=(0.0, -1.0, 2.5))
    b.material("matte", Kd=(0.6, 0.55, 0.5))
    quad(b, (-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0))
    b.material("matte", Kd=(0.4, 0.5, 0.6))
    quad(b, (-4, 4, 0), (4, 4, 0), (4, 4, 4), (-4, 4, 4))
    for i, (x, y, z) in enumerate(((2.5, 1.0, 2.0), (-2.6, 0.5, 1.5), (0.3, 2.5, 3.0), (-1.0, -1.5, 2.2), (1.4, -0.8, 1.2))):
        triangle_light(b, z=z, L=(4.0 + i, 5.0, 8.0 - i), half=0.3, at=(x, y))
    b.attribute_begin(); b.material("matte", Kd=(0, 0, 0)); b.area_light_source("diffuse", L=(5, 5, 4)); b.translate((-0.5, 1.2, 1.0))
    b.shape("sphere", radius=0.35); b.attribute_end()
    cam = PerspectiveCamera.look_at(be, (0.2, -5.5, 2.0), (0.0, 0.5, 1.2), (0, 0, 1), res, fov=50.0)
    return b, cam, res


# ------------------------------------------------------------------ configurations
class Config:
    """floor: the value metric's floor, a hundredth of the largest radiance a light of the scene gives a surface (written next to each configuration,
    from the scene's description; never from results)"""

    def __init__(self, name, make, kind, depth, rr, spp, seed, floor, error=0):
        self.name, self.make, self.kind, self.depth, self.rr, self.spp, self.seed, self.floor, self.error = name, make, kind, depth, rr, spp, seed, floor, error

    def integrator(self):
        return {"path": lambda: PathIntegrator(self.depth, self.rr), "direct": lambda: DirectLightingIntegrator(self.depth), "whitted": lambda: WhittedIntegrator(self.depth)}[self.kind]()

    def sampler(self, first=0, count=0):
        return RandomSampler(self.spp, self.seed, indexed=True, first_sample=first, sample_count=count)


U = A.FTN_ERR_UNSUPPORTED
_C = [
    # the closed box: L = 12 -> 0.12
    Config("box_d0", closed_box, "path", 0, 1.0, 4, 11, 0.12), Config("box_d1", closed_box, "path", 1, 1.0, 4, 12, 0.12), Config("box_d2", closed_box, "path", 2, 1.0, 4, 13, 0.12),
    Config("box_d5", closed_box, "path", 5, 1.0, 4, 14, 0.12), Config("box_d5_rr0", closed_box, "path", 5, 0.0, 4, 15, 0.12),
    Config("box_direct", closed_box, "direct", 3, 0.0, 4, 16, 0.12), Config("box_whitted", closed_box, "whitted", 3, 0.0, 4, 17, 0.12),
    Config("dim_box_d12", lambda be: closed_box(be, albedo=0.45), "path", 12, 1.0, 8, 18, 0.12),
    Config("dented_path", dented_box, "path", 3, 1.0, 4, 81, 0.12), Config("dented_direct", dented_box, "direct", 2, 0.0, 4, 82, 0.12),
    Config("dented_whitted", dented_box, "whitted", 2, 0.0, 4, 83, 0.12),
    # every material, a point (I = 40 at 3 or more: 4.4), a distant (1.5) and an area light (8); thin lens -> 0.08
    Config("materials_path", materials_small, "path", 2, 1.0, 4, 21, 0.08), Config("materials_direct", materials_small, "direct", 3, 0.0, 4, 22, 0.08),
    Config("materials_whitted", materials_small, "whitted", 3, 0.0, 4, 23, 0.08),
    # the same materials and lights on spheres that are only translated: on a rotated or scaled sphere the reference's normals (transform.rs:133-139 as
    # written) are off, offset_ray_origin then leaves the ray inside the sphere's error interval, and long chains there exceed the share left out
    Config("gallery_path", gallery, "path", 5, 1.0, 4, 71, 0.08), Config("gallery_direct", gallery, "direct", 4, 0.0, 4, 72, 0.08),
    Config("gallery_whitted", gallery, "whitted", 4, 0.0, 4, 73, 0.08),
    # scenes.cornell: L = 15 -> 0.15; scenes.furnace: L = 1 -> 0.01
    Config("cornell_path", lambda be: scenes.cornell(be, res=16), "path", 5, 1.0, 4, 24, 0.15), Config("cornell_direct", lambda be: scenes.cornell(be, res=16), "direct", 4, 0.0, 4, 25, 0.15),
    Config("cornell_whitted", lambda be: scenes.cornell(be, res=16), "whitted", 4, 0.0, 4, 26, 0.15),
    Config("furnace_path", lambda be: scenes.furnace(be, res=16), "path", 6, 1.0, 4, 27, 0.01), Config("furnace_direct", lambda be: scenes.furnace(be, res=16), "direct", 3, 0.0, 4, 28, 0.01),
    # environment maps: texels up to 1.5 x 6 = 9 -> 0.09
    Config("env8_path", lambda be: env_boxes(be, 8, 8, False), "path", 3, 1.0, 4, 31, 0.09), Config("env8_direct", lambda be: env_boxes(be, 8, 8, False), "direct", 2, 0.0, 4, 32, 0.09),
    Config("env33_path", lambda be: env_boxes(be, 33, 16, False), "path", 3, 1.0, 4, 33, 0.09), Config("env33_area_path", lambda be: env_boxes(be, 33, 16, True), "path", 3, 1.0, 4, 34, 0.09),
    Config("env8_area_direct", lambda be: env_boxes(be, 8, 8, True), "direct", 2, 0.0, 4, 35, 0.09), Config("env8_area_whitted", lambda be: env_boxes(be, 8, 8, True), "whitted", 2, 0.0, 4, 36, 0.09),
    # the partial sphere: L = 9 -> 0.09
    Config("lamp_path", sphere_lamp, "path", 3, 1.0, 4, 41, 0.09), Config("lamp_direct", sphere_lamp, "direct", 2, 0.0, 4, 42, 0.09), Config("lamp_whitted", sphere_lamp, "whitted", 2, 0.0, 4, 43, 0.09),
    # the corridor: L = 10 -> 0.1
    Config("corridor_path", mirror_corridor, "path", 6, 1.0, 4, 44, 0.1), Config("corridor_direct", mirror_corridor, "direct", 5, 0.0, 4, 45, 0.1),
    Config("corridor_whitted", mirror_corridor, "whitted", 5, 0.0, 4, 46, 0.1),
    # the sheet without a material
    Config("sheet_path", lambda be: closed_box(be, sheet=True), "path", 3, 1.0, 4, 51, 0.12), Config("sheet_direct", lambda be: closed_box(be, sheet=True), "direct", 3, 0.0, 4, 52, 0.12, error=U),
    Config("sheet_whitted", lambda be: closed_box(be, sheet=True), "whitted", 3, 0.0, 4, 53, 0.12, error=U),
    # no light at all (the floor has nothing to come from; every value must be exactly 0)
    Config("dark_path", lambda be: closed_box(be, light=False), "path", 3, 1.0, 4, 54, 1.0), Config("dark_direct", lambda be: closed_box(be, light=False), "direct", 3, 0.0, 4, 55, 1.0),
    # textures: the point light gives the floor I / r^2 = 14 / 2.2^2 = 2.9, the triangle 7 -> 0.07
    Config("checker_path", lambda be: textured_room(be, False), "path", 3, 1.0, 4, 61, 0.07), Config("checker_direct", lambda be: textured_room(be, False), "direct", 3, 0.0, 4, 62, 0.07),
    Config("image_path", lambda be: textured_room(be, True), "path", 3, 1.0, 4, 63, 0.07), Config("image_direct", lambda be: textured_room(be, True), "direct", 3, 0.0, 4, 64, 0.07),
    # six emitters and a point light: L up to 8 -> 0.08
    Config("emitters_direct", emitters, "direct", 1, 0.0, 4, 91, 0.08),
]
CONFIGS = {c.name: c for c in _C}

# Measured on the CPU, libm oracle against the restatement: (99.9th percentile, maximum) of the value metric and the share of samples left out.
# The bounds are 4 x these.  None comes from the device.
MEASURED = {
    "box_d0": (0.000e+00, 0.000e+00, 0.000000),
    "box_d1": (1.934e-06, 2.464e-06, 0.000000),
    "box_d2": (3.661e-06, 7.688e-06, 0.000000),
    "box_d5": (4.127e-06, 6.717e-06, 0.000000),
    "box_d5_rr0": (3.086e-06, 3.916e-06, 0.000000),
    "box_direct": (3.833e-06, 7.782e-06, 0.000000),
    "box_whitted": (5.437e-06, 6.146e-06, 0.000000),
    "dim_box_d12": (1.996e-06, 4.981e-06, 0.000000),
    "dented_path": (1.854e-06, 2.501e-06, 0.000000),
    "dented_direct": (6.258e-07, 7.556e-07, 0.000000),
    "dented_whitted": (6.914e-07, 8.211e-07, 0.000000),
    "materials_path": (6.266e-05, 1.774e-04, 0.014974),
    "materials_direct": (1.356e-04, 2.646e-04, 0.004557),
    "materials_whitted": (8.802e-05, 1.483e-04, 0.009115),
    "gallery_path": (1.404e-04, 7.808e-04, 0.000000),
    "gallery_direct": (1.133e-04, 2.856e-04, 0.001302),
    "gallery_whitted": (1.093e-04, 1.601e-04, 0.000000),
    "cornell_path": (8.566e-05, 7.246e-04, 0.001953),
    "cornell_direct": (6.802e-05, 9.614e-05, 0.001953),
    "cornell_whitted": (7.061e-05, 8.662e-05, 0.000977),
    "furnace_path": (7.335e-07, 9.314e-07, 0.000977),
    "furnace_direct": (1.636e-07, 2.341e-07, 0.000000),
    "env8_path": (1.948e-05, 3.045e-05, 0.000781),
    "env8_direct": (3.844e-05, 7.676e-05, 0.000781),
    "env33_path": (7.024e-06, 1.935e-05, 0.000781),
    "env33_area_path": (6.736e-06, 5.367e-05, 0.000000),
    "env8_area_direct": (6.751e-06, 1.132e-05, 0.000781),
    "env8_area_whitted": (3.642e-06, 6.640e-06, 0.001563),
    "lamp_path": (1.199e-04, 2.823e-04, 0.002344),
    "lamp_direct": (2.763e-04, 1.155e-03, 0.002344),
    "lamp_whitted": (4.887e-05, 9.865e-05, 0.000000),
    "corridor_path": (5.828e-07, 6.319e-07, 0.000000),
    "corridor_direct": (6.012e-07, 7.610e-07, 0.000977),
    "corridor_whitted": (4.154e-07, 6.979e-07, 0.000977),
    "sheet_path": (3.070e-06, 1.363e-05, 0.000000),
    "dark_path": (0.000e+00, 0.000e+00, 0.000000),
    "dark_direct": (0.000e+00, 0.000e+00, 0.000000),
    "checker_path": (1.768e-05, 4.425e-05, 0.000000),
    "checker_direct": (4.931e-06, 5.450e-06, 0.000000),
    "image_path": (7.425e-06, 8.405e-06, 0.000000),
    "image_direct": (1.077e-05, 1.780e-05, 0.000000),
    "emitters_direct": (6.167e-04, 6.885e-04, 0.000977),
}
TOLERANCE = {k: (4.0 * v[0], 4.0 * v[1]) for k, v in MEASURED.items()}


# ------------------------------------------------------------------ one sample at a time
def area_order(scene):
    """the emitting primitives (the builder's indices) in the order of Scene::lights: the BVH's primitive order (scene/mod.rs:38-42)"""
    _, prim = scene.lights()
    order = scene.nodes()[1]
    return [int(order[p]) for p in prim if p >= 0]


def key(px, py, s):
    return (np.asarray(py, np.int64) * 65536 + np.asarray(px, np.int64)) * 65536 + np.asarray(s, np.int64)


@functools.lru_cache(maxsize=None)
def restated(name):
    """the restatement of a configuration, computed once per session (pixels row-major, samples increasing)"""
    from oracle_loader import oracle_backend
    cfg = CONFIGS[name]
    be = oracle_backend(det=False)                    # only to hold the description; nothing a library computes is read but Scene::lights' order
    b, cam, res = cfg.make(be)
    order = None
    if sum(1 for p in b.prims for _ in range(p[2] if p[0] == "trirange" else 1) if p[-1] >= 0) > 1:
        order = area_order(b.create_scene())
    ref = IG.render(b, cam, res, cfg.spp, cfg.seed, cfg.kind, cfg.depth, cfg.rr, area_order=order)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def logged(orc, cfg):
    """the oracle's sample log in the restatement's order -> records, stats; FountainError as the library raises it"""
    b, cam, res = cfg.make(orc)
    rec, st = MR.sample_log(orc, b.create_scene(), cam, GR.film(orc, res), cfg.integrator(), cfg.sampler())
    return rec[np.argsort(key(rec["px"], rec["py"], rec["sample"]))], st


def one_sample_films(be, cfg, setting=None, make=None):
    """every camera sample through one-sample ranges on a box film of radius 0.5 -> xyz [n, 3] float32 (pixels row-major, samples increasing),
    the summed statistics.  Asserts that no sample spilled and that every pixel's weight is 1."""
    b, cam, res = (make or cfg.make)(be)
    scene = b.create_scene()
    kw = dict(SETTINGS[setting]) if setting else dict(count_traffic=True)
    out = np.zeros((res[1], res[0], cfg.spp, 3), F32)
    total = {}
    for s in range(cfg.spp):
        film = GR.film(be, res)
        st = SamplerIntegrator(cam, cfg.integrator()).render_parallel(scene, film, cfg.sampler(s, 1), **kw)
        assert st["spill_samples"] == 0 and st["camera_samples"] == res[0] * res[1], (cfg.name, s, st)
        assert np.all(film.pixels[..., 3] == 1.0)
        out[:, :, s] = film.pixels[..., :3]
        for k in ("rays_closest", "rays_any", "camera_samples"):
            total[k] = total.get(k, 0) + st[k]
    return out.reshape(-1, 3), total


def error_code(fn):
    try:
        fn()
    except FountainError as e:
        return e.code
    return 0


# ------------------------------------------------------------------ layer 1: the comparison
def compare(cfg, ref, rec):
    """a library's sample log (in the restatement's order) against the restatement -> (99.9th percentile, maximum of the value metric, share of samples
    left out).  Asserts the discrete outcomes: the set of samples, p_film bit for bit, ray_weight, black on both sides or on neither."""
    assert np.array_equal(key(rec["px"], rec["py"], rec["sample"]), key(ref["px"], ref["py"], ref["sample"])), cfg.name + ": another set of samples"
    assert np.array_equal(GR.bits(rec["p_film"]), GR.bits(ref["p_film"])), cfg.name + ": p_film"
    assert np.array_equal(rec["ray_weight"], ref["ray_weight"]), cfg.name + ": ray_weight"
    keep = ~ref["fragile"]
    got, want = rec["L"].astype(np.float64), ref["L"]
    assert np.isfinite(got).all() and (got >= 0.0).all(), cfg.name
    differs = IG.black(got) != IG.black(want)
    assert not differs[keep].any(), (cfg.name, "black on one side only", int(differs[keep].sum()), np.flatnonzero(differs & keep)[:8])
    e = (np.abs(got - want) / np.maximum(np.abs(want), cfg.floor))[keep]
    share = float(ref["fragile"].mean())
    if not e.size:
        return 0.0, 0.0, share
    return float(np.percentile(e, 99.9)), float(e.max()), share


def ray_counts_agree(cfg, ref, st):
    """the ray counts of a render against the restatement's, up to what the samples left out can move"""
    for k in ("rays_closest", "rays_any"):
        slack = int(ref[k][ref["fragile"]].sum()) + int(ref["fragile"].sum()) * 2 * (cfg.depth + 2)
        assert abs(int(st[k]) - int(ref[k].sum())) <= slack, (cfg.name, k, st[k], int(ref[k].sum()), slack)


# ------------------------------------------------------------------ layer 2: properties no reading of the reference enters
def scaled(make, k):
    """the scene of `make` with every light's L / I, every environment texel and every area emission multiplied by k (a power of two)"""
    def build(be):
        b, cam, res = make(be)
        for l in b.lights:
            for c in range(3):
                l.rgb[c] = float(F32(l.rgb[c]) * F32(k))
        b.envmaps = [(t * F32(k)).astype(F32) for t in b.envmaps]
        b.area_emit = [tuple(float(F32(x) * F32(k)) for x in e) for e in b.area_emit]
        return b, cam, res
    return build


SCALING = ["box_d5", "gallery_path", "gallery_direct", "gallery_whitted", "env33_area_path", "lamp_direct", "image_path"]
SCALES = (2.0, 0.125)


def check_exact_scaling(cfg, render):
    """render(make) -> (values [..] float32, stats): the values of the scaled scenes are the scaled values bit for bit (a power of two commutes with
    every rounding short of underflow; roulette, the choice of light and all pdfs depend on throughput and geometry only), the ray counts equal"""
    base, st = render(cfg.make)
    assert np.any(base != 0)
    for k in SCALES:
        got, st_k = render(scaled(cfg.make, k))
        assert np.array_equal(GR.bits(got), GR.bits(base * F32(k))), (cfg.name, k, int((GR.bits(got) != GR.bits(base * F32(k))).sum()))
        for c in ("rays_closest", "rays_any", "camera_samples"):
            assert st_k[c] == st[c], (cfg.name, k, c)


def per_pixel(rec, res):
    """a sample log -> per-pixel mean [h, w, 3] and variance of that mean (binary64)"""
    n = len(rec) // (res[0] * res[1])
    L = rec["L"].astype(np.float64).reshape(res[1], res[0], n, 3)
    return L.mean(axis=2), L.var(axis=2, ddof=1) / n


def oracle_pixels(orc, make, integ, spp, seed):
    b, cam, res = make(orc)
    rec, st = MR.sample_log(orc, b.create_scene(), cam, GR.film(orc, res), integ, RandomSampler(spp, seed, indexed=True))
    rec = rec[np.argsort(key(rec["px"], rec["py"], rec["sample"]))]
    assert np.isfinite(rec["L"]).all() and (rec["L"] >= 0).all()
    mean, var = per_pixel(rec, res)
    return mean, var, st


def device_pixels(gpu, make, integ, spp, seed, setting):
    """per-pixel mean from a render through `setting`; the variance of that mean from ftn_render_moments (its one-pass binary32 formula, pinned by
    test_moments_oracle.py), which runs on the wavefront pipeline only: for the megakernel its counting build stands in (the samples are the same)"""
    from fountain_amd import moments as M
    b, cam, res = make(gpu)
    scene = b.create_scene()
    smp = RandomSampler(spp, seed, indexed=True)
    film = GR.film(gpu, res)
    st = SamplerIntegrator(cam, integ).render_parallel(scene, film, smp, **SETTINGS[setting])
    rgb, _ = film.into_spectrum_buffer()
    assert np.isfinite(rgb).all() and (rgb >= 0).all()
    var = M.render_moments(gpu, None, cam, res, integ, smp, scene=scene, film=GR.film(gpu, res), pipeline=WAVE, count_traffic=SETTINGS[setting]["count_traffic"])[0]
    return rgb.astype(np.float64), var[..., :3].astype(np.float64), st


ROUNDING = 1.0e-5       # what a dozen binary32 operations and a binary32 sum of samples may move a mean by, relative: the allowance where sigma is 0


def check_means(name, mean, var, expect, quadrature_moves):
    """every pixel mean and the image mean within 5 sigma of the quadrature; doubling the quadrature's nodes moves it by less than a tenth of that"""
    allowed = 5.0 * np.sqrt(var) + ROUNDING * np.abs(expect)
    assert (quadrature_moves <= 0.1 * allowed).all(), (name, "the quadrature has not converged", float((quadrature_moves / allowed).max()))
    z = np.abs(mean - expect) / allowed
    assert (z <= 1.0).all(), (name, "a pixel mean", float(z.max()))
    n = mean.shape[0] * mean.shape[1]
    m, e = mean.mean(axis=(0, 1)), expect.mean(axis=(0, 1))
    s = np.sqrt(var.sum(axis=(0, 1))) / n
    assert (np.abs(m - e) <= 5.0 * s + ROUNDING * e).all(), (name, "the image mean", m, e, s)
    return float((5.0 * s / e).max())


def gauss_legendre(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w


KD = (0.6, 0.5, 0.4)
LIT = {"point": dict(I=(30.0, 28.0, 25.0), p=(1.0, 0.5, 2.0)), "distant": dict(L=(2.0, 1.8, 1.5), frm=(1.0, -1.0, 2.0)),
       "sphere": dict(L=(6.0, 5.5, 5.0), c=(1.5, 1.0, 2.5), R=0.8), "env": dict(L=(0.8, 0.9, 1.0))}
RECEIVERS = {"matte": ("matte", dict(Kd=KD)), "plastic": ("plastic", dict(Kd=(0.3, 0.25, 0.2), Ks=(0.5, 0.5, 0.5), roughness=0.1)),
             "metal": ("metal", dict(eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14), uroughness=0.08, vroughness=0.3))}


MIS_RES, MIS_FOV = (64, 4), 5.0                       # four tiles side by side (the oracle renders tiles in parallel), a narrow view


def lit_floor(be, light, receiver="matte", res=(16, 16), R=None, fov=40.0):
    """one big triangle as the floor, seen from above, unoccluded, under one light the camera does not see"""
    b = SceneBuilder(be)
    d = LIT[light]
    if light == "point":
        b.light_source("point", I=d["I"], from_=d["p"])
    elif light == "distant":
        b.light_source("distant", L=d["L"], from_=d["frm"], to=(0, 0, 0))
    elif light == "env":
        b.light_source("infinite", L=d["L"])
    else:
        b.attribute_begin(); b.material("matte", Kd=(0, 0, 0)); b.area_light_source("diffuse", L=d["L"]); b.translate(d["c"]); b.shape("sphere", radius=R or d["R"]); b.attribute_end()
    name, kw = RECEIVERS[receiver]
    b.material(name, **kw)
    b.shape("trianglemesh", P=[(-30, -20, 0), (30, -20, 0), (0, 40, 0)], indices=[0, 1, 2])
    cam = PerspectiveCamera.look_at(be, (0.3, -0.2, 3.0), (0.0, 0.0, 0.0), (0, 1, 0), res, fov=fov)
    return b, cam, res


def mis_floor(receiver, R):
    return lambda be: lit_floor(be, "sphere", receiver, MIS_RES, R, MIS_FOV)


def floor_hits(make, n):
    """the floor interactions of n x n Gauss-Legendre nodes of every pixel's jitter square through the restated camera -> S, weights [n * n]"""
    from oracle_loader import oracle_backend
    b, cam, res = make(oracle_backend(det=False))
    x, w = gauss_legendre(n)
    py, px, j, i = np.meshgrid(np.arange(res[1]), np.arange(res[0]), np.arange(n), np.arange(n), indexing="ij")
    rows = np.stack([(px + x[i]).ravel(), (py + x[j]).ravel()] + [np.zeros(px.size)] * 3, axis=1)
    ray = IR.camera(cam.desc, 1, rows)
    sc = IG.SceneRef(b)
    S = sc.intersect(ray["o"], ray["d"])
    assert S["hit"].all() and (sc.mat[S["prim"]] >= 0).all()
    return sc, S, np.outer(w, w).ravel(), res


def expected_matte(light, n):
    """Kd / pi x the irradiance in closed form, averaged over each pixel's jitter square with n x n nodes"""
    sc, S, w, res = floor_hits(lambda be: lit_floor(be, light), n)
    d = LIT[light]
    p = S["p"]
    if light == "point":
        v = np.array(d["p"]) - p
        r2 = IG.dot(v, v)
        E = np.array(d["I"])[None] * (v[:, 2] / np.sqrt(r2) / r2)[:, None]
    elif light == "distant":
        wl = np.array(d["frm"]) / np.linalg.norm(d["frm"])
        E = np.array(d["L"])[None] * np.full(len(p), wl[2])[:, None]
    elif light == "sphere":
        v = np.array(d["c"]) - p
        r2 = IG.dot(v, v)
        E = np.pi * np.array(d["L"])[None] * (d["R"] ** 2 / r2 * v[:, 2] / np.sqrt(r2))[:, None]
    else:
        E = np.pi * np.array(d["L"])[None] * np.ones(len(p))[:, None]
    L = np.array(KD, np.float32).astype(np.float64) / np.pi * E
    return (L.reshape(res[1], res[0], len(w), 3) * w[None, None, :, None]).sum(axis=2)


def expected_glossy(receiver, R, n, m):
    """the integral of f cos L over the sphere light's cone (m x 2m nodes in (cos alpha, phi)) with _bsdf_ref's f at the restated floor interaction,
    averaged over each pixel's jitter square (n x n nodes)"""
    sc, S, w, res = floor_hits(mis_floor(receiver, R), n)
    d = LIT["sphere"]
    name, kw = RECEIVERS[receiver]
    lobes = B.material_lobes(name, True, **kw)
    v = np.array(d["c"]) - S["p"]
    dist = np.sqrt(IG.dot(v, v))
    axis = v / dist[:, None]
    e1, e2 = IR.coordinate_system(axis)
    cos_max = np.sqrt(1.0 - (R / dist) ** 2)
    xc, wc = gauss_legendre(m)
    phi = (np.arange(2 * m) + 0.5) * (np.pi / m)
    out = np.zeros((len(dist), 3))
    bsdf = B.Bsdf(lobes, S["n"], S["ns"], S["s_dpdu"])
    for a, wa in zip(xc, wc):
        ca = 1.0 - a * (1.0 - cos_max)                # cos alpha from 1 to cos_max: d omega = d(cos alpha) d phi
        sa = np.sqrt(1.0 - ca * ca)
        for ph in phi:
            wi = axis * ca[:, None] + (e1 * np.cos(ph) + e2 * np.sin(ph)) * sa[:, None]
            f = bsdf.f(S["wo"], wi, B.ALL)
            out += f * (np.abs(IG.dot(wi, S["ns"])) * wa * (1.0 - cos_max) * (np.pi / m))[:, None]
    out *= np.array(d["L"])[None]
    return (out.reshape(res[1], res[0], len(w), 3) * w[None, None, :, None]).sum(axis=2)


@functools.lru_cache(maxsize=None)
def quadrature(what, *args):
    """(expected [h, w, 3], how far doubling the nodes moves it), once per session"""
    if what == "matte":
        a, b = expected_matte(args[0], 4), expected_matte(args[0], 8)
    else:
        a, b = expected_glossy(args[0], args[1], 1, 12), expected_glossy(args[0], args[1], 2, 24)
    return b, np.abs(b - a)


# Sample counts chosen on the CPU with the libm oracle so that 5 sigma of the image mean is at most 0.5 % of it (asserted; DESIGN.md 3.5 records the
# measured sigma).  Per-pixel sigma comes from the samples themselves, so no count is below 64 (5 sigma of a Student t with 63 degrees).
MEAN_SHARE = 0.005
MEAN_CASES = {"point": 64, "distant": 64, "sphere": 14336, "env": 288}
MIS_CASES = {("plastic", 0.15): 10240, ("plastic", 1.0): 14336, ("metal", 0.15): 14336, ("metal", 1.0): 23552}
MEAN_INTEGRATORS = {"direct": lambda: DirectLightingIntegrator(1), "path": lambda: PathIntegrator(1, 0.0), "whitted": lambda: WhittedIntegrator(1)}
MEAN_PARAMS = [(l, i) for l in MEAN_CASES for i in MEAN_INTEGRATORS if i != "whitted" or l in ("point", "distant")]      # Whitted: the two delta lights
MIS_PARAMS = [(r, R, i) for (r, R) in MIS_CASES for i in ("direct", "path")]


def check_mean_case(pixels, light, integ):
    """pixels(make, integrator, spp, seed) -> mean, variance of the mean, stats"""
    expect, moves = quadrature("matte", light)
    mean, var, _ = pixels(lambda be: lit_floor(be, light), MEAN_INTEGRATORS[integ](), MEAN_CASES[light], 5)
    share = check_means("%s/%s" % (light, integ), mean, var, expect, moves)
    assert share <= MEAN_SHARE, (light, integ, share)
    return share


def check_mis_case(pixels, receiver, R, integ):
    expect, moves = quadrature("glossy", receiver, R)
    mean, var, _ = pixels(mis_floor(receiver, R), MEAN_INTEGRATORS[integ](), MIS_CASES[(receiver, R)], 7)
    share = check_means("%s/%s/%s" % (receiver, R, integ), mean, var, expect, moves)
    assert share <= MEAN_SHARE, (receiver, R, integ, share)
    return share


def check_estimators_agree(pixels):
    """PathIntegrator(1, 0.0) and DirectLightingIntegrator(1) on the closed box, independent seeds: per-pixel means within 5 sigma of their difference"""
    a, va, _ = pixels(closed_box, PathIntegrator(1, 0.0), 128, 91)
    b, vb, _ = pixels(closed_box, DirectLightingIntegrator(1), 128, 92)
    s = np.sqrt(va + vb)
    assert (np.abs(a - b) <= 5.0 * s + ROUNDING * np.abs(a)).all(), float((np.abs(a - b) / (5.0 * s + ROUNDING * np.abs(a) + 1e-300)).max())
    assert (s > 0).any() and a.mean() > 0.05


def check_roulette_unbiased(pixels):
    """the low-albedo box at depth 12: rr_threshold 1.0 against 0.0, independent seeds; paths were cut (fewer rays), the image means agree within 5 sigma
    and so does every pixel"""
    make = lambda be: closed_box(be, albedo=0.45)
    a, va, sa = pixels(make, PathIntegrator(12, 1.0), 256, 93)
    b, vb, sb = pixels(make, PathIntegrator(12, 0.0), 256, 94)
    assert sa["rays_closest"] < sb["rays_closest"]
    s = np.sqrt(va + vb)
    assert (np.abs(a - b) <= 5.0 * s + ROUNDING * np.abs(a)).all()
    n = a.shape[0] * a.shape[1]
    assert (np.abs(a.mean(axis=(0, 1)) - b.mean(axis=(0, 1))) <= 5.0 * np.sqrt((va + vb).sum(axis=(0, 1))) / n).all()
