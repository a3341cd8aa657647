"""The oracle's light code (oracle/orc_scene.hpp, orc_shapes.hpp through orc_test_light) against tests/_light_ref.py, an independent binary64
restatement of the reference's Rust, and against properties no reading of the reference enters: sample / pdf agreement, where the samples
go, the estimator's integral against closed forms, sanity.  Runs without a GPU, on the libm oracle and on the deterministic-math one;
tests/test_light.py reruns the properties on the device through the same helpers (tests/_light_common.py).  DESIGN.md 3.2."""
import numpy as np
import pytest

import _light_common as K
import _light_ref as R

_hooks = {}


@pytest.fixture(params=["libm", "det"])
def oracle(request, orc, orc_det):
    be = orc if request.param == "libm" else orc_det

    def get(name, among=False):
        key = (request.param, name, among)
        if key not in _hooks:
            _hooks[key] = K.Hook(be, name, among=among)
        return _hooks[key]
    get.be = be
    return get


@pytest.mark.parametrize("name", K.ALL_NAMES)
def test_oracle_matches_the_restatement(oracle, name):
    """Dense random rows: reference points spread around the light, u in [0, 1)^2, wi half random and half aimed at the light.  Discrete outcomes
    identical (a pdf is 0 on both sides or on neither: sample accepted, hit or miss of pdf_from_ref; a CDF cell off would move wi by a cell),
    values within the measured tolerance (K.TOL_P999 at the 99.9th percentile, K.TOL_MAX at the maximum), at most 0.5 % of the rows left out
    because binary32 rounding may flip a branch.  Infinite lights also as one of several lights."""
    for among in ((False, True) if name in K.ENV_MAPS else (False,)):
        hook = oracle(name, among)
        err, left_out = K.compare_with_restatement(hook, K.random_rows(hook.desc, 1000, 100000))
        p999, worst = float(np.quantile(err, 0.999)), float(err.max())
        print("restatement %-20s among %d: p99.9 %.3e max %.3e left out %.4f" % (name, among, p999, worst, left_out))
        assert left_out <= K.MAX_FRAGILE_SHARE, (name, left_out)
        assert p999 <= K.TOL_P999 and worst <= K.TOL_MAX, (name, p999, worst)


@pytest.mark.parametrize("name", K.DELTAS + list(K.TRIANGLES) + list(K.SPHERES) + K.WELL_FORMED_ENVS)
def test_sample_and_pdf_agree(oracle, name):
    K.check_sample_pdf_agreement(oracle(name))


@pytest.mark.parametrize("name", K.DELTAS + list(K.TRIANGLES) + list(K.SPHERES) + K.WELL_FORMED_ENVS)
def test_sanity(oracle, name):
    K.check_sanity(oracle(name))


@pytest.mark.parametrize("name", K.HIST_CASES)
def test_samples_go_where_the_light_is(oracle, name):
    K.check_histogram(oracle(name))


@pytest.mark.parametrize("name", K.EST_CASES)
def test_estimator_integrates_to_the_closed_form(oracle, name):
    K.check_estimator(oracle(name))


# ---- quirks of the reference, reproduced and pinned
def test_far_side_sphere_sample_gets_the_near_hits_pdf(oracle):
    K.check_far_side_sphere_quirk(oracle("sph_full"))


def test_zero_map_pdf_is_pdf_zero(oracle):
    K.check_zero_map_pdf_quirk(oracle("env_plateau"))


def test_search_below_the_first_entry_ends_in_cell_zero(oracle):
    K.check_search_underflow_quirk(oracle("env_sq33"))


def test_black_map_gives_nan_pdfs(oracle):
    K.check_black_map_quirk(oracle("env_zero"))


@pytest.mark.parametrize("name", ["env_sq33", "env_64x33"])
def test_pdf_at_the_south_pole_is_negative(oracle, name):
    K.check_south_pole_quirk(oracle(name))


def test_normals_are_transformed_by_the_inverse_not_its_transpose(oracle):
    """transform.rs:133-139 multiplies a normal by the inverse matrix where its comment promises the inverse's transpose.  Under a rotation or a
    non-uniform scale the sampled normal of a sphere is therefore not the surface's: reproduced, not fixed (found by the restatement)."""
    hook = oracle("sph_scaled")
    s = hook.desc["shape"]
    rows = K.random_rows(hook.desc, 47, 2000)
    o = hook(rows)
    smp = s.sample(rows[:, 13:15].astype(np.float64))
    true_n = R.normalize(smp["obj"] @ s.o2w_inv[:3, :3])
    got = o["p1_n"].astype(np.float64)
    assert np.abs(got - smp["n"]).max() <= 1.0e-5
    assert np.median(np.abs(R.dot(got, true_n))) < 0.9


def test_hook_refuses_bad_arguments(oracle):
    K.check_refusals(oracle.be, via_env0_refused=False)


# ---- the edge table of tests/test_light.py does what it is for
@pytest.mark.parametrize("name", [k for k in K.WELL_FORMED_ENVS if k != "env_uniform"])
def test_cdf_windows_straddle_the_entries(oracle, name):
    checked = K.check_env_table_reaches_its_edges(oracle(name))
    dist = oracle(name).desc["env"].distribution
    assert len(checked) >= (dist.nu + dist.nv) // 4 or name in ("env_sq2", "env_3x5"), (name, len(checked))
    if name in ("env_sq33", "env_sq40", "env_sq64", "env_sq65", "env_sq128", "env_33x64", "env_64x33", "env_plateau"):
        assert any(k % 32 == 0 for _, k in checked), name                            # a block boundary of the coarse table, hit exactly


def test_edge_table_reaches_the_edges(orc_det):
    """a plateau crossed, a cell fall-back taken, a NaN pdf from a NaN direction, pdf 0 at the poles, a far-side sphere sample"""
    hook = K.Hook(orc_det, "env_plateau")
    desc = hook.desc
    a, b, row = K.env_cdf_rows(desc)
    w = 2 * K.CDF_WINDOW + 1
    _, y, _ = K.env_cell_coordinates(desc, hook(a)["wi"])
    y32 = y[32 * w:33 * w]                             # u.y around the marginal's entry 32, inside its plateau 30..36
    assert np.any(np.abs(y32 - 30.0) < 0.01) and np.any(np.abs(y32 - 36.0) < 0.01) and np.all((np.abs(y32 - 30.0) < 0.01) | (np.abs(y32 - 36.0) < 0.01))
    x, _, _ = K.env_cell_coordinates(desc, hook(b)["wi"])
    x64 = x[64 * w:65 * w]                             # u.x around the conditional's entry 64 = 1: the top of cell 59, or the last cell
    assert np.any(np.abs(x64 - 60.0) < 0.01) and np.any(np.abs(x64 - 64.0) < 0.01)
    rows = K.edge_rows(desc)
    o = hook(rows)
    nan_wi = np.isnan(rows[:, 10:13]).any(axis=1)
    assert nan_wi.any() and np.all(np.isnan(o["pdf_in"][nan_wi]))
    pole = (rows[:, 10] == 0.0) & (rows[:, 11] == 0.0) & (rows[:, 12] == 1.0)
    assert pole.any() and np.all(o["pdf_in"][pole] == 0.0)
    # the cell fall-back of the device's records: a sample whose 2 x 2 lookup block (mipmap.rs:268-271) does not start at its cell or the one before,
    # which takes a u beyond [0, 1) -- by the restatement's sampled cell and (d0, d1)
    want = R.evaluate(desc, rows)
    with np.errstate(all="ignore"):
        dx = np.floor(want["uv"][:, 0] * desc["env"].w - 0.5) - want["cell"][:, 0]
        dy = np.floor(want["uv"][:, 1] * desc["env"].h - 0.5) - want["cell"][:, 1]
    outside = np.isfinite(dx) & np.isfinite(dy) & ((dx < -1) | (dx > 0) | (dy < -1) | (dy > 0))
    inside = np.isfinite(dx) & np.isfinite(dy) & ~outside
    assert outside.sum() >= 20 and inside.sum() >= 1000 and np.isnan(dx).sum() >= 10
    for v in (-1.0, 0.0):                              # every corner of the record's 3 x 3 neighbourhood is read
        for h in (-1.0, 0.0):
            assert np.any(inside & (dx == v) & (dy == h))
    # area lights: the table's samples reach the far side of a sphere
    sph = K.Hook(orc_det, "sph_full")
    rows = K.edge_rows(sph.desc)
    want = R.evaluate(sph.desc, rows)
    o = sph(rows)
    far = (want["which_s"] == 0) & want["hit_s"] & (o["radiance"][:, 0] == 0.0) & (o["pdf"] > 0.0) & ~want["fragile"]
    assert far.sum() >= 10
