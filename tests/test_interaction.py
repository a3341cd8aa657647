"""The device's surface interactions and ray differentials (ftn_device.h: tri_hit, tri_interaction, sphere_intersect, make_interaction, spawn_ray,
camera_ray; ftn_texture.h: compute_tex_diffs, camera_ray_diff, specular_diff; through ftn_test_interaction and ftn_test_camera) bit for bit against
the deterministic-math oracle on dense random rows and on an explicit table of edges, under the three data paths of a triangle, against the
production entry points on the same rays, and against the properties of tests/test_interaction_cpu.py (same helpers, seeds and bounds:
tests/_interaction_common.py), so that a change to the device code cannot hide behind an oracle that changed with it.  DESIGN.md 3.3."""
import numpy as np
import pytest

import _interaction_common as K
from fountain_amd import FountainError

pytestmark = pytest.mark.gpu
f32 = np.float32
CASES = [(name, variant) for name in K.ALL_NAMES for variant in K.variants_of(name)]
CASE_IDS = ["%s-%s" % c for c in CASES]
_hooks, _want = {}, {}


@pytest.fixture
def dev(gpu, monkeypatch):
    def get(name, variant=None):
        variant = variant or K.variants_of(name)[0]
        if (name, variant) not in _hooks:
            _hooks[(name, variant)] = K.Hook(gpu, name, variant, monkeypatch)
        return _hooks[(name, variant)]
    return get


@pytest.fixture
def ref(orc_det):
    def get(name, variant=None):
        key = ("ref", name, variant == "dense")
        if key not in _hooks:
            _hooks[key] = K.Hook(orc_det, name, "dense" if variant == "dense" else K.variants_of(name)[0])
        return _hooks[key]
    return get


def oracle_rows(ref, name, variant, what, rows):
    """the oracle's output, computed once per (configuration, scene, table) and shared by the build variants"""
    key = (name, variant == "dense", what)
    if key not in _want:
        if len(_want) >= 4:
            _want.pop(next(iter(_want)))
        _want[key] = ref(name, variant).raw(rows)
    return _want[key]


def assert_same(got, want, rows, what, geo=None):
    same = K.same_bits_or_both_nan(got, want)
    if geo is not None and not same.all():            # (the edge table alone: rays that overflow the triangle test)
        loose = K.undefined_by_the_reference(geo, rows)
        assert loose.sum() <= K.MAX_UNDEFINED_SHARE * len(rows), (what, int(loose.sum()))
        same |= loose[:, None]
    if not same.all():
        bad = np.argwhere(~same)
        lines = ["row %d column %d: device %r oracle %r, input %r" % (r, c, got[r, c], want[r, c], rows[r].tolist()) for r, c in bad[:6]]
        raise AssertionError("%s: %d rows differ; columns %s\n%s" % (what, int((~same).any(axis=1).sum()), sorted(set(bad[:, 1].tolist())), "\n".join(lines)))


@pytest.mark.parametrize("name,variant", CASES, ids=CASE_IDS)
def test_device_matches_oracle_on_random_rows(dev, ref, name, variant):
    """2 x 10^5 rows per configuration and data path"""
    d = dev(name, variant)
    assert d.order.tolist() == ref(name, variant).order.tolist()
    rows = K.random_rows(d.targets, 2000, 200000)
    assert not K.undefined_by_the_reference(d.targets, rows).any()
    assert_same(d.raw(rows), oracle_rows(ref, name, variant, "random", rows), rows, "%s %s" % (name, variant))


@pytest.mark.parametrize("name,variant", CASES, ids=CASE_IDS)
def test_device_matches_oracle_on_the_edge_table(dev, ref, name, variant):
    d = dev(name, variant)
    rows = K.edge_rows(d.targets)
    assert_same(d.raw(rows), oracle_rows(ref, name, variant, "edges", rows), rows, "%s %s" % (name, variant), geo=d.targets)


@pytest.mark.parametrize("name", list(K.TRIANGLES))
def test_three_data_paths_give_the_same_rows(dev, name):
    """shading records, FTN_SREC=0 (indexed arrays) and the dense `geom` array beside a sphere: the same bits (the dense scene has one more primitive,
    which no row names)"""
    rows = np.concatenate([K.random_rows(dev(name, "srec").targets, 2001, 50000), K.edge_rows(dev(name, "srec").targets)])
    outs = {v: dev(name, v).raw(rows) for v in K.variants_of(name)}
    assert (outs["srec"][:, 0] != 0.0).sum() > 1000
    assert_same(outs["no_srec"], outs["srec"], rows, name + " without shading records")
    assert_same(outs["dense"], outs["srec"], rows, name + " beside a sphere")


@pytest.mark.parametrize("name,variant", CASES, ids=CASE_IDS)
def test_hook_agrees_with_the_production_entry_points(dev, name, variant):
    """on the same scene and rays, aimed so that at most one primitive is in the way: t and the barycentrics of ftn_intersect(stats=False) and the DSI
    columns of ftn_intersect_full, bit for bit (two triangles sharing an edge: the rows that name the primitive the closest hit is on)"""
    d = dev(name, variant)
    rows = K.random_rows(d.targets, 2002, 50000)
    rows[:, 6] = np.where(np.isfinite(rows[:, 6]), rows[:, 6], np.inf)
    out = d.raw(rows)
    t, prim, bary, _ = d.scene.intersect(rows[:, 0:8], stats=False)
    full = d.scene.intersect_full(rows[:, 0:8])
    named = d.to_bvh[K.prim_of(rows)]
    hit = out[:, 0] != 0.0
    closest = prim == named
    if len(d.targets) == 1:
        assert np.array_equal(hit, prim >= 0), (name, int(hit.sum()), int((prim >= 0).sum()))
    else:
        assert not np.any(closest & ~hit)
    m = hit & closest
    assert m.sum() > 2000
    assert K.same_bits_or_both_nan(out[m, 1], t[m]).all() and K.same_bits_or_both_nan(out[m, 2:5], bary[m]).all()
    assert K.same_bits_or_both_nan(full[m, 23], t[m]).all()
    for a, b in ((slice(5, 14), slice(0, 9)), (slice(15, 18), slice(11, 14)), (slice(21, 24), slice(14, 17)), (slice(18, 21), slice(20, 23))):   # p p_err n | wo | shading dpdu | ns
        assert K.same_bits_or_both_nan(out[m, a], full[m, b]).all(), (name, a)


PROPERTY_CHECKS = [K.check_error_box, K.check_spawned_ray_leaves, K.check_frames, K.check_derivatives, K.check_texture_differentials, K.check_sanity]


@pytest.mark.parametrize("name", K.ALL_NAMES)
@pytest.mark.parametrize("check", PROPERTY_CHECKS, ids=[c.__name__[6:] for c in PROPERTY_CHECKS])
def test_properties(dev, check, name):
    check(dev(name))


@pytest.mark.parametrize("name", K.ALL_NAMES)
def test_primitive_order_is_a_bijection(dev, name):
    for variant in K.variants_of(name):
        K.check_primitive_mapping(dev(name, variant))


@pytest.mark.parametrize("name", K.BOUNCE_NAMES)
def test_reflected_differential_lacks_a_factor_two(dev, name):
    for side in (1.0, -1.0):
        K.check_bounced_differential(dev(name), True, side)


@pytest.mark.parametrize("name", K.TRANSMIT_NAMES)
def test_transmitted_differential_has_the_sign_of_cos_t_and_the_unflipped_normal(dev, name):
    for side in (1.0, -1.0):
        K.check_bounced_differential(dev(name), False, side)


def test_scaled_sphere_normal_disagrees_with_the_surface(dev):
    assert abs(K.check_spawned_ray_leaves(dev("sph_scaled")) - K.SCALED_SPHERE_DISAGREEMENT) <= 0.002
    for name in K.TRANSLATED_SPHERES:
        assert K.check_spawned_ray_leaves(dev(name)) == 0.0, name


@pytest.mark.parametrize("name", K.CAMERA_NAMES)
def test_camera_matches_oracle(gpu, orc_det, name):
    """10^5 random rows and the table of film corners, lens edges and shutter ends, per camera and samples-per-pixel count"""
    rows = np.concatenate([K.camera_rows(name, 2003, 100000), K.camera_edge_rows(name)])
    for spp in K.SPPS:
        got = K.camera_raw(gpu, K.cameras(gpu)[name][0], spp, rows)
        want = K.camera_raw(orc_det, K.cameras(orc_det)[name][0], spp, rows)
        same = K.same_bits_or_both_nan(got, want)
        assert same.all(), (name, spp, np.argwhere(~same)[:5].tolist())


@pytest.mark.parametrize("name", K.CAMERA_NAMES)
def test_camera_properties(gpu, name):
    K.check_camera(gpu, name)


def test_lens_rays_meet_the_plane_of_focus(gpu):
    K.check_lens_focus(gpu)


def test_hook_refuses_bad_arguments(gpu):
    K.check_refusals(gpu)
    cam = K.cameras(gpu)["pinhole"][0]
    with pytest.raises(FountainError):
        K.camera_raw(gpu, cam, 0, K.camera_rows("pinhole", 1, 4))
    assert K.camera_raw(gpu, cam, 4, np.zeros((0, K.CIN), f32)).shape == (0, K.COUT)
