"""The device's BVH and traversal kernels (k_wf_trace4, k_wf_trace4<.., Q64>, k_wf_trace4_any, k_wf_trace8_any and the reference-order k_wf_trace)
through ftn_intersect / ftn_intersect_test / ftn_intersect_full: against brute force over every primitive in binary64, against the
deterministic oracle bit for bit under every knob that selects another kernel or another stack, for independence of the batch a ray arrives in, and the
invariants of the device-resident tree and light list.  tests/test_traversal_cpu.py holds both oracle builds to the same rules."""
import numpy as np
import pytest

import _traversal_common as T
import _traversal_ref as TR

pytestmark = pytest.mark.gpu

KNOBS = {
    "default": {},
    "quad64_off": {"FTN_QUAD64": "0"},                # closest hit over the 128-byte records
    "t8_off": {"FTN_T8": "0"},                        # any hit over the four-box records
    "trace4_off": {"FTN_TRACE4": "0"},                # the two-record kernels
    "one_entry": {"FTN_T4_ENTRIES": "1", "FTN_T4_ENTRIES_ANY": "1", "FTN_T8_ENTRIES": "1"},          # every push but the first spills
    "sorted": {"FTN_WF_SORT": "1"},
    "batch_simple": {"FTN_BATCH_SIMPLE": "1"},        # one lane per ray, the plain loop
}
ALL_KNOBS = sorted({k for env in KNOBS.values() for k in env})


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def families(name):
    return T.FAMILIES + (["seams"] if name in T.SEAM_SCENES else [])


def all_rays(name):
    if name == "ulp_apart":                           # no families of its own: rays through its box
        return np.ascontiguousarray(T.rays("one", "random")[:512] * np.float32(0.5) + np.array([1, 0.5, 0.5, 0, 0, 0, 0, 0], np.float32))
    if name == "tie":
        return np.concatenate([T.exact_rays()[0], T.rays("grid", "random")[:512], T.rays("grid", "axis")[:256]])
    return np.concatenate([T.rays(name, f) for f in families(name)])


_scene, _oracle = {}, {}


def device_scene(gpu, name):
    """the scene under the default knobs, created once"""
    if name not in _scene:
        _scene[name] = T.build(gpu, name).create_scene()
    return _scene[name]


def oracle_rows(orc_det, name):
    """the deterministic oracle on every ray of the scene, computed once -> t, prim (BVH index), occluded, the full records"""
    if name not in _oracle:
        sc = T.build(orc_det, name).create_scene()
        rays = all_rays(name)
        t, prim, _, _ = sc.intersect(rays)
        _oracle[name] = (t, prim, sc.intersect_test(rays)[0], sc.intersect_full(rays), sc.nodes())
    return _oracle[name]


@pytest.fixture
def clean_knobs(monkeypatch):
    for k in ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


# ------------------------------------------------------------------ 1. against brute force
@pytest.mark.parametrize("name,family", [(s, f) for s in T.SCENES for f in families(s)])
def test_device_against_brute_force(gpu, clean_knobs, name, family):
    """the production kernels (stats=False) and the counting build of the reference-order walk (stats=True) under the layer-B rules, on every row"""
    sc = device_scene(gpu, name)
    order = sc.nodes()[1]
    rays = T.rays(name, family)
    J = TR.judgement(name, family)
    for stats in (False, True):
        what = (name, family, "counting" if stats else "production")
        t, prim, bary, _ = sc.intersect(rays, stats=stats)
        occ, _ = sc.intersect_test(rays, stats=stats)
        pb = TR.builder_index(prim, order)
        ratio = TR.check_closest(J, t, pb, what, bary=bary)
        TR.check_occluded(J, occ, pb, what)
        assert ratio <= 4.0 * T.MEASURED[name][0], (what, ratio)
        if family == "seams":
            TR.check_seams(J, T.description(name)[1], rays, t, pb, occ, T.seam_faces(name), what)
    if family in T.PINNED_FAMILIES:
        assert J.pinned.mean() >= T.MIN_PINNED[name]


@pytest.mark.parametrize("knobs", sorted(KNOBS))
def test_exact_rays(gpu, clean_knobs, knobs):
    """where binary32 rounds nothing the reference's text decides (_traversal_common.exact_rays), under every knob, production and counting build"""
    for k, v in KNOBS[knobs].items():
        clean_knobs.setenv(k, v)
    sc = T.build(gpu, "tie").create_scene()
    rays = T.exact_rays()[0]
    for stats in (False, True):
        t, prim, _, _ = sc.intersect(rays, stats=stats)
        T.check_exact(t, prim, sc.intersect_test(rays, stats=stats)[0], sc.nodes()[1], (knobs, stats))


# ------------------------------------------------------------------ 2. against the deterministic oracle, bit for bit
@pytest.mark.parametrize("name", T.TREE_SCENES)
@pytest.mark.parametrize("knobs", sorted(KNOBS))
def test_device_equals_the_oracle(gpu, orc_det, clean_knobs, knobs, name):
    to, po, oo, fo, _ = oracle_rows(orc_det, name)
    rays = all_rays(name)
    base = device_scene(gpu, name).info()
    for k, v in KNOBS[knobs].items():                 # before create_scene(): the records are built at creation
        clean_knobs.setenv(k, v)
    sc = T.build(gpu, name).create_scene()
    info = sc.info()
    has_records = name in T.TRIANGLE_ONLY and name != "one"          # an interior node, no sphere: the eight-box tree and the 64-byte records exist
    assert (info["oct_bytes"] > 0) == has_records, (name, info["oct_bytes"])
    if knobs == "quad64_off":
        assert (info["quad_bytes"] < base["quad_bytes"]) == has_records, (name, info["quad_bytes"], base["quad_bytes"])
    else:
        assert info["quad_bytes"] == base["quad_bytes"]
    t, prim, bary, none = sc.intersect(rays, stats=False)
    assert none is None
    occ, _ = sc.intersect_test(rays, stats=False)
    assert np.array_equal(bits(t), bits(to)) and np.array_equal(prim, po), (knobs, name, "closest hit", np.flatnonzero((bits(t) != bits(to)) | (prim != po))[:8])
    assert np.array_equal(occ, oo), (knobs, name, "any hit", np.flatnonzero(occ != oo)[:8])
    tc, pc, bc, _ = sc.intersect(rays)
    occ_c, _ = sc.intersect_test(rays)
    assert np.array_equal(bits(tc), bits(to)) and np.array_equal(pc, po) and np.array_equal(occ_c, oo), (knobs, name, "counting build")
    assert np.array_equal(bits(bary), bits(bc)), (knobs, name, "barycentrics")
    full = sc.intersect_full(rays)
    for sl in (slice(0, 9), slice(11, 17), slice(20, 24)):          # p, p_err, n | wo, shading dpdu | shading_n, t  (uv and dpdv: the oracle only)
        assert np.array_equal(bits(full[:, sl]), bits(fo[:, sl])), (knobs, name, "full records", sl)


# ------------------------------------------------------------------ 3. a ray's result does not depend on the batch it arrives in
SIZES = (1, 2, 63, 64, 65, 511, 512, 513, 577, 4095, 4096)


@pytest.mark.parametrize("name", ["comb", "shared_box", "cube600"])
def test_batch_independence(gpu, clean_knobs, name):
    """the per-wave chunks and the eight XCD slices of wq_refill are cut with & ~63: prefixes around those cuts, a permutation and a repetition of one
    4097-ray batch return the same bits, for closest hit, any hit and the full records"""
    sc = device_scene(gpu, name)
    rays = T.batch_mix(name)
    assert len(rays) == 4097

    def run(r):
        t, prim, bary, _ = sc.intersect(r, stats=False)
        return [bits(t), prim, bits(bary), sc.intersect_test(r, stats=False)[0], bits(sc.intersect_full(r))]

    whole = run(rays)
    assert 0 < (whole[1] >= 0).sum() < len(rays) and 0 < whole[3].sum() < len(rays)
    for n in SIZES:
        for a, b in zip(run(rays[:n]), whole):
            assert np.array_equal(a, b[:n]), (name, n)
    perm = np.random.default_rng(9).permutation(len(rays))
    for a, b in zip(run(np.ascontiguousarray(rays[perm])), whole):
        assert np.array_equal(a, b[perm]), (name, "permuted")
    for a, b in zip(run(rays), whole):
        assert np.array_equal(a, b), (name, "twice")


# ------------------------------------------------------------------ 4. the device-resident tree and light list
@pytest.mark.parametrize("name", T.TREE_SCENES)
def test_device_tree_and_lights(gpu, orc_det, clean_knobs, name):
    sc = device_scene(gpu, name)
    b = T.description(name)[0]
    nodes, order = sc.nodes()
    TR.check_tree(b, nodes, order, sc.info()["max_depth"])
    kind, prim = sc.lights()
    got = TR.check_lights(b, kind, prim, order)
    if name == "emitters":
        assert len(got) == 6 and got != sorted(got)
    on, oo = oracle_rows(orc_det, name)[4]
    assert nodes.tobytes() == on.tobytes() and np.array_equal(order, oo)
