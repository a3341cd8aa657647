"""The oracle's texture path (oracle/orc_texture.hpp through orc_test_texture_eval, orc_test_material and orc_test_mipmap_level) against
tests/_texture_ref.py, an independent binary64 restatement of the reference, and against properties that no reading of the reference enters.
Both oracle builds: the libm one sets the tolerances, the deterministic-math one is what the device is compared with bit for bit;
tests/test_texture.py reruns the properties on the device through the same helpers (tests/_texture_common.py).  DESIGN.md 3.4."""
import numpy as np
import pytest

import _texture_common as K
import _texture_ref as X

_hooks = {}
BUILDS = ["libm", "det"]


@pytest.fixture
def hook(orc, orc_det):
    def get(build, name):
        if (build, name) not in _hooks:
            _hooks[(build, name)] = K.Hook(orc if build == "libm" else orc_det, name)
        return _hooks[(build, name)]
    return get


# ---- layer 1: the restatement
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", K.SCENES)
def test_oracle_matches_the_restatement(hook, build, name):
    """10^5 random rows per texture and material: identical discrete outcomes, values within 4 x the measured figures, at most 0.5 % of the rows left out"""
    h = hook(build, name)
    for i, target in enumerate(h.targets()):
        p999, worst, share = K.compare_with_restatement(h, target, K.random_rows(1000 + i))
        print("%s %s %s: p99.9 %.3g max %.3g left out %.5f" % (build, name, target[1], p999, worst, share))
        assert share <= X.MAX_FRAGILE_SHARE, (name, target, share)
        bp, bm = K.bound(K.MEASURED, name + "/" + target[1])
        assert p999 <= bp and worst <= bm, (name, target, p999, worst)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", ["img_12x20", "img_17x33"])
def test_oracle_matches_the_restatement_far_from_the_origin(hook, build, name):
    """uv of 10^3 ... 10^5: binary32 keeps 24 bits of st * w, so the position inside a texel is lost from about 10^5 on -- a bound of its own"""
    h = hook(build, name)
    for i, target in enumerate(h.targets()):
        p999, worst, share = K.compare_with_restatement(h, target, K.far_rows(2000 + i))
        print("%s %s %s far: p99.9 %.3g max %.3g left out %.5f" % (build, name, target[1], p999, worst, share))
        assert share <= X.MAX_FRAGILE_SHARE, (name, target, share)
        bp, bm = K.bound(K.MEASURED_FAR, name + "/" + target[1])
        assert p999 <= bp and worst <= bm, (name, target, p999, worst)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", K.IMAGE_SCENES)
def test_edge_table_matches_the_restatement(hook, build, name):
    """the edge table of tests/test_texture.py, row by row, unless fragile: NaN and infinities must agree, the rest within its own measured bound
    (at +-1e10 the bilinear weights are of that size and cancel)"""
    h = hook(build, name)
    rows = K.edge_rows(h.stored("id_repeat")[0].shape[:2])
    far = K.beyond_binary32(rows)
    for wrap in K.WRAPS:
        err, fragile = K.errors_against_restatement(h, ("tex", "id_" + wrap), rows)
        for table, select, what in ((K.MEASURED_EDGE, ~far, "edge"), (K.MEASURED_EDGE_1E10, far, "edge at 1e10")):
            p999, worst, share = K.summary(err, fragile, select)
            print("%s %s %s %s (%d rows): p99.9 %.3g max %.3g left out %.5f" % (build, name, wrap, what, select.sum(), p999, worst, share))
            assert share <= K.MAX_EDGE_FRAGILE_SHARE, (name, wrap, share)
            bp, bm = K.bound(table, name + "/" + wrap)
            assert p999 <= bp and worst <= bm, (name, wrap, what, p999, worst)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", K.IMAGE_SCENES + ["special"])
def test_pyramid_levels_match_the_restatement(hook, build, name):
    h = hook(build, name)
    for k in K.image_textures(h):
        if k.startswith(("nan_", "huge_")):
            continue
        e = K.compare_levels(h, k)
        print("%s %s %s levels: %.3g" % (build, name, k, e))
        assert e <= K.TOL_FACTOR * K.MEASURED_LEVELS, (name, k, e)


def test_sixteen_levels_at_the_size_limit(hook):
    h = hook("det", "img_1x32768")
    levels = h.levels("id_repeat")
    assert [l.shape[:2] for l in levels] == [(1, 32768 >> l) for l in range(16)]


# ---- layer 2: properties
@pytest.mark.parametrize("build", BUILDS)
def test_constant_image_reads_back(hook, build):
    K.check_constant_image(hook(build, "const"))


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", K.IMAGE_SCENES)
def test_image_properties(hook, build, name):
    h = hook(build, name)
    K.check_range(h)
    K.check_periodic(h)
    K.check_outside(h)
    K.check_top_texel(h)
    K.check_integer_levels(h)
    K.check_continuity_in_width(h)


@pytest.mark.parametrize("build", BUILDS)
def test_affine_ramp_is_reproduced(hook, build):
    K.check_ramp(hook(build, "special"))


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", ["img_5x4", "img_17x33", "img_1x1"])
def test_lookup_trilinear_takes_dst0_y_without_abs(hook, build, name):
    """quirk, reproduced (mipmap.rs, lookup_trilinear: `dst0.x.abs().max(dst0.y)`)"""
    K.check_quirk_dst0_y(hook(build, name))


@pytest.mark.parametrize("build", BUILDS)
def test_float_checkerboard_takes_its_two_values(hook, build):
    K.check_float_checkerboard(hook(build, "procedural"))


@pytest.mark.parametrize("build", BUILDS)
def test_material_from_equal_children_is_the_material_from_constants(hook, build):
    K.check_same_constant(hook(build, "same"))


@pytest.mark.parametrize("build", BUILDS)
def test_material_finalising(hook, build):
    K.check_finalising(hook(build, "mats"))


@pytest.mark.parametrize("build", BUILDS)
def test_untextured_material_comes_back_as_uploaded(hook, build):
    K.check_untextured(hook(build, "mats"), hook(build, "mats_plain"))
    K.check_untextured(hook(build, "mats_plain"))


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", K.SCENES)
def test_outputs_are_finite(hook, build, name):
    K.check_finite(hook(build, name))


def test_hook_refuses_bad_arguments(hook, orc_det):
    K.check_refusals(orc_det, hook("det", "mats"))


def test_edge_table_reaches_the_edges():
    rows = K.edge_rows((17, 33))
    uv = rows[:, :2]
    assert np.isnan(uv).any() and np.isinf(uv).any() and (np.abs(uv) == 1.0e10).any() and (uv.view(np.uint32) == 0x80000000).any()
    assert ((uv != 0) & (np.abs(uv) < 1.0e-38)).any() and (uv == np.float32(16.5 / 33)).any() and (uv == np.float32(4 / 8)).any()
    w = 2 * np.abs(rows[:, 2:]).max(axis=1)
    for v in (0.0, 1.0, 10.0, 2.0 ** -5, 2.0 ** -16):
        assert (w == np.float32(v)).any(), v
    assert (rows[:, 2:] < 0).any() and (rows[:, 2:] > 0).any()
