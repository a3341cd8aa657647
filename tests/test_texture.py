"""The device's texture path (ftn_texture.h: tex_eval, mip_lookup_trilinear*, mip_triangle, mip_texel, material_resolve -> material_finalize;
build_mip_pyramid of the host driver; through ftn_test_texture_eval, ftn_test_material and ftn_test_mipmap_level) bit for bit against the
deterministic-math oracle on every configuration and on an edge table per image, against the independent restatement within the bounds
measured on the CPU, and against the properties of tests/_texture_common.py -- the same code, seeds and bounds tests/test_texture_cpu.py runs
on both oracle builds.  DESIGN.md 3.4."""
import numpy as np
import pytest

import _texture_common as K
import _texture_ref as X
from fountain_amd import FountainError, PathIntegrator, RandomSampler, SceneBuilder, _abi as A, scenes

pytestmark = pytest.mark.gpu
_hooks = {}


@pytest.fixture
def hook(gpu, orc_det):
    def get(side, name):
        if (side, name) not in _hooks:
            _hooks[(side, name)] = K.Hook(gpu if side == "gpu" else orc_det, name)
        return _hooks[(side, name)]
    return get


def equal(a, b):
    """the same bits, or NaN on both sides (which NaN an invalid operation returns is the hardware's choice: tests/test_bsdf.py, _light_common.py)"""
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def same_bits(a, b):
    return a.shape == b.shape and bool(equal(a, b).all())


# ---- layer 3: bit for bit
@pytest.mark.parametrize("name", K.SCENES)
def test_device_equals_the_oracle(hook, name):
    """every texture and material of every scene: 10^5 random rows, rows far from the origin, and (images) the edge table"""
    g, o = hook("gpu", name), hook("det", name)
    for i, target in enumerate(g.targets()):
        rows = np.concatenate([K.random_rows(1000 + i), K.far_rows(2000 + i, 5000)])
        assert same_bits(g.run(target, rows), o.run(target, rows)), (name, target)
    if name in K.IMAGE_SCENES:
        rows = K.edge_rows(g.stored("id_repeat")[0].shape[:2])
        for k in g.tex:
            a, b = g.eval(k, rows), o.eval(k, rows)
            bad = np.flatnonzero(~equal(a, b).all(axis=1))
            assert bad.size == 0, (name, k, bad.size, rows[bad[:4]], a[bad[:4]], b[bad[:4]])


@pytest.mark.parametrize("name", K.IMAGE_SCENES + ["special"])
def test_host_pyramid_equals_the_oracle(hook, name):
    g, o = hook("gpu", name), hook("det", name)
    for k in K.image_textures(g):
        a, b = g.levels(k), o.levels(k)
        assert len(a) == len(b) and all(x.shape == y.shape and same_bits(x, y) for x, y in zip(a, b)), (name, k)


# ---- layer 1 on the device: the restatement, within the bounds the libm oracle set
@pytest.mark.parametrize("name", K.SCENES)
def test_device_matches_the_restatement(hook, name):
    h = hook("gpu", name)
    for i, target in enumerate(h.targets()):
        p999, worst, share = K.compare_with_restatement(h, target, K.random_rows(1000 + i))
        print("gpu %s %s: p99.9 %.3g max %.3g left out %.5f" % (name, target[1], p999, worst, share))
        assert share <= X.MAX_FRAGILE_SHARE, (name, target, share)
        bp, bm = K.bound(K.MEASURED, name + "/" + target[1])
        assert p999 <= bp and worst <= bm, (name, target, p999, worst)


# ---- layer 2: properties
def test_constant_image_reads_back(hook):
    K.check_constant_image(hook("gpu", "const"))


@pytest.mark.parametrize("name", K.IMAGE_SCENES)
def test_image_properties(hook, name):
    h = hook("gpu", name)
    K.check_range(h)
    K.check_periodic(h)
    K.check_outside(h)
    K.check_top_texel(h)
    K.check_integer_levels(h)
    K.check_continuity_in_width(h)


def test_affine_ramp_is_reproduced(hook):
    K.check_ramp(hook("gpu", "special"))


@pytest.mark.parametrize("name", ["img_5x4", "img_17x33", "img_1x1"])
def test_lookup_trilinear_takes_dst0_y_without_abs(hook, name):
    """quirk, reproduced (mipmap.rs, lookup_trilinear: `dst0.x.abs().max(dst0.y)`)"""
    K.check_quirk_dst0_y(hook("gpu", name))


def test_float_checkerboard_takes_its_two_values(hook):
    K.check_float_checkerboard(hook("gpu", "procedural"))


def test_material_from_equal_children_is_the_material_from_constants(hook):
    K.check_same_constant(hook("gpu", "same"))


def test_material_finalising(hook):
    K.check_finalising(hook("gpu", "mats"))


def test_untextured_material_comes_back_as_uploaded(hook):
    K.check_untextured(hook("gpu", "mats"), hook("gpu", "mats_plain"))
    K.check_untextured(hook("gpu", "mats_plain"))


@pytest.mark.parametrize("name", K.SCENES)
def test_outputs_are_finite(hook, name):
    K.check_finite(hook("gpu", name))


def test_hook_refuses_bad_arguments(gpu, hook):
    K.check_refusals(gpu, hook("gpu", "mats"))


# ---- the upper size limit
def test_image_past_the_size_limit_is_refused_and_the_device_goes_on(gpu, orc_det, hook):
    """1 x 32768 builds the 16 levels DImage has room for; 1 x 65536 would need 17 and is refused with FTN_ERR_UNSUPPORTED, and the next scene
    on the same device renders as ever"""
    assert len(hook("gpu", "img_1x32768").levels("id_repeat")) == 16
    b = SceneBuilder(gpu)
    b.texture("wide", "spectrum", "imagemap", texels=np.full((1, 65536, 3), 0.5, np.float32))
    b.material("matte", Kd="wide")
    b.shape("sphere")
    with pytest.raises(FountainError) as e:
        b.create_scene()
    assert e.value.code == A.FTN_ERR_UNSUPPORTED
    films = []
    for be in (gpu, orc_det):
        sb, cam, res = scenes.cornell(be, res=16)
        films.append(scenes.render(be, sb, cam, res, PathIntegrator(3, 1.0), RandomSampler(2, 0, indexed=True))[1])
    assert np.allclose(films[0], films[1], rtol=1e-6, atol=1e-7) and films[0].std() > 0
