"""The device's light code (ftn_device.h: light_sample, light_pdf, light_sample_env, light_pdf_env, light_Le_env, area_Le, shape_sample,
shape_pdf_from_ref, the blocked CDF search and the env cell records, through ftn_test_light) bit for bit against the deterministic-math
oracle, on dense random rows and on an explicit table of edges, under every build variant and through both routes to the same code, and
against the properties of tests/test_light_cpu.py (same helpers, seeds and bounds: tests/_light_common.py), so that a change to the
device code cannot hide behind an oracle that changed with it.  DESIGN.md 3.2."""
import ctypes as C

import numpy as np
import pytest

import _light_common as K
from fountain_amd import _abi as A

pytestmark = pytest.mark.gpu
f32 = np.float32
CASES = [(name, variant) for name in K.ALL_NAMES for variant in K.variants_of(name)]
CASE_IDS = ["%s-%s" % c for c in CASES]
_hooks, _want = {}, {}


@pytest.fixture
def dev(gpu, monkeypatch):
    def get(name, variant="default", among=False):
        key = (name, variant, among)
        if key not in _hooks:
            _hooks[key] = K.Hook(gpu, name, variant, among, monkeypatch)
        return _hooks[key]
    return get


@pytest.fixture
def ref(orc_det):
    def get(name, variant="default", among=False):
        key = ("ref", name, variant == "dense", among)
        if key not in _hooks:
            _hooks[key] = K.Hook(orc_det, name, variant, among)
        return _hooks[key]
    return get


def oracle_rows(ref, name, variant, among, what, rows):
    """the oracle's output, computed once per (configuration, scene, table) and shared by the build variants"""
    key = (name, variant == "dense", among, what)
    if key not in _want:
        if len(_want) >= 4:
            _want.pop(next(iter(_want)))
        _want[key] = ref(name, variant, among).raw(rows)
    return _want[key]


def assert_same(got, want, rows, what, desc=None):
    same = K.same_bits_or_both_nan(got, want)
    if desc is not None and not same.all():           # (the edge table alone; K.undefined_by_the_reference says which rows it can touch)
        mask = K.undefined_by_the_reference(desc, rows, got, want)
        assert mask.any(axis=1).sum() <= K.MAX_UNDEFINED_SHARE * len(rows), (what, int(mask.any(axis=1).sum()))
        same |= mask
    if not same.all():
        bad = np.argwhere(~same)
        lines = ["row %d column %d: device %r oracle %r, input %r" % (r, c, got[r, c], want[r, c], rows[r].tolist()) for r, c in bad[:6]]
        raise AssertionError("%s: %d rows differ; columns %s\n%s" % (what, int((~same).any(axis=1).sum()), sorted(set(bad[:, 1].tolist())), "\n".join(lines)))


def compare(dev, ref, name, variant, what, rows_of, strict=False):
    for among in ((False, True) if name in K.ENV_MAPS else (False,)):
        d = dev(name, variant, among)
        rows = rows_of(d.desc)
        want = oracle_rows(ref, name, variant, among, what, rows)
        assert_same(d.raw(rows), want, rows, "%s %s among %d" % (name, variant, among), None if strict else d.desc)
        if name in K.ENV_MAPS and not among:           # the copy of the light in the kernel arguments: the route of the shading kernels
            assert_same(d.raw(rows, via_env0=1), want, rows, "%s %s via env0" % (name, variant))


@pytest.mark.parametrize("name,variant", CASES, ids=CASE_IDS)
def test_device_matches_oracle_on_random_rows(dev, ref, name, variant):
    """2 x 10^5 rows per configuration and build variant; infinite lights as the only light through both routes, and as one of several"""
    compare(dev, ref, name, variant, "random", lambda desc: K.random_rows(desc, 2000, 200000), strict=True)


@pytest.mark.parametrize("name,variant", CASES, ids=CASE_IDS)
def test_device_matches_oracle_on_the_edge_table(dev, ref, name, variant):
    compare(dev, ref, name, variant, "edges", K.edge_rows)


@pytest.mark.parametrize("name", [k for k in K.SQUARE_ENVS if k in K.MONOTONE_ENVS])
def test_blocked_search_and_cell_records_change_nothing(dev, name):
    """the CDF-entry table under the default build (coarse tables, cell records), without the coarse tables and without the cell records: the
    same rows, bit for bit (in addition to the comparison of each with the oracle above)"""
    rows = None
    outs = {}
    for variant in K.ENV_VARIANTS:
        d = dev(name, variant)
        if rows is None:
            a, b, _ = K.env_cdf_rows(d.desc)
            rows = np.concatenate([a, b])
        outs[variant] = d.raw(rows)
    assert_same(outs["no_coarse"], outs["default"], rows, name + " without the coarse tables")
    assert_same(outs["no_cells"], outs["no_coarse"], rows, name + " without the cell records")


PROPERTY_NAMES = K.DELTAS + list(K.TRIANGLES) + list(K.SPHERES) + K.WELL_FORMED_ENVS


@pytest.mark.parametrize("name", PROPERTY_NAMES)
def test_sample_and_pdf_agree(dev, name):
    K.check_sample_pdf_agreement(dev(name, K.variants_of(name)[0]))


@pytest.mark.parametrize("name", PROPERTY_NAMES)
def test_sanity(dev, name):
    K.check_sanity(dev(name, K.variants_of(name)[0]))


@pytest.mark.parametrize("name", K.HIST_CASES)
def test_samples_go_where_the_light_is(dev, name):
    K.check_histogram(dev(name, K.variants_of(name)[0]))


@pytest.mark.parametrize("name", K.EST_CASES)
def test_estimator_integrates_to_the_closed_form(dev, name):
    K.check_estimator(dev(name, K.variants_of(name)[0]))


def test_far_side_sphere_sample_gets_the_near_hits_pdf(dev):
    K.check_far_side_sphere_quirk(dev("sph_full"))


def test_zero_map_pdf_is_pdf_zero(dev):
    for variant in K.ENV_VARIANTS:
        K.check_zero_map_pdf_quirk(dev("env_plateau", variant))


def test_search_below_the_first_entry_ends_in_cell_zero(dev):
    K.check_search_underflow_quirk(dev("env_sq33"))


def test_black_map_gives_nan_pdfs(dev):
    K.check_black_map_quirk(dev("env_zero"))


@pytest.mark.parametrize("name", ["env_sq33", "env_64x33"])
def test_pdf_at_the_south_pole_is_negative(dev, name):
    K.check_south_pole_quirk(dev(name))


def test_hook_refuses_bad_arguments(gpu):
    from fountain_amd import FountainError
    for rc in K.check_refusals(gpu):
        with pytest.raises(FountainError):
            gpu.check(rc)
