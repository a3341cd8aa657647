"""Shared by tests/test_bsdf_cpu.py (the oracle) and tests/test_bsdf.py (the device): the material configurations, the rows fed
to the BSDF hook, the measured tolerances and the property checks, so that both sides face the same seeds and the same bounds."""
import ctypes as C

import numpy as np

import _bsdf_ref as R
from _rows import run_rows
from fountain_amd import SceneBuilder, _abi as A

f32 = np.float32
ALL = A.BSDF_ALL
FLAG_SETS = [ALL, ALL & ~A.BSDF_SPECULAR, A.BSDF_REFLECTION | A.BSDF_SPECULAR, A.BSDF_TRANSMISSION | A.BSDF_SPECULAR,
             A.BSDF_REFLECTION | A.BSDF_DIFFUSE, 0]      # everything, all but specular, reflection|specular, transmission|specular, diffuse only, none
NON_SPECULAR = ALL & ~A.BSDF_SPECULAR

GOLD = dict(eta=(0.2, 0.9, 1.1), k=(3.9, 2.4, 2.2))
CONFIGS = [
    ("matte_lambert", "matte", dict(Kd=(0.5, 0.4, 0.3), sigma=0.0)),
    ("matte_sigma20", "matte", dict(Kd=(0.5, 0.4, 0.3), sigma=20.0)),
    ("matte_sigma90", "matte", dict(Kd=(0.5, 0.4, 0.3), sigma=90.0)),
    ("matte_negative", "matte", dict(Kd=(0.5, -0.2, 0.3), sigma=20.0)),
    ("matte_black", "matte", dict(Kd=(0.0, 0.0, 0.0), sigma=0.0)),
    ("mirror", "mirror", dict(Kr=(0.9, 0.8, 0.7))),
    ("plastic_kd", "plastic", dict(Kd=(0.3, 0.2, 0.1), Ks=(0.0, 0.0, 0.0), roughness=0.1)),
    ("plastic_ks", "plastic", dict(Kd=(0.0, 0.0, 0.0), Ks=(0.3, 0.4, 0.5), roughness=0.2, remaproughness=False)),
    ("plastic_both", "plastic", dict(Kd=(0.3, 0.2, 0.1), Ks=(0.3, 0.4, 0.5), roughness=0.1, remaproughness=True)),
    ("plastic_both_noremap", "plastic", dict(Kd=(0.3, 0.2, 0.1), Ks=(0.3, 0.4, 0.5), roughness=0.3, remaproughness=False)),
    ("metal_iso", "metal", dict(roughness=0.3, remaproughness=False, **GOLD)),
    ("metal_iso_remap", "metal", dict(roughness=0.05, remaproughness=True, **GOLD)),
    ("metal_aniso_uv", "metal", dict(uroughness=0.05, vroughness=0.4, remaproughness=False, **GOLD)),
    ("metal_aniso_vu", "metal", dict(uroughness=0.4, vroughness=0.05, remaproughness=False, **GOLD)),
    ("glass_rough", "glass", dict(Kr=(0.9, 0.9, 0.8), Kt=(0.8, 0.9, 0.9), eta=1.5, uroughness=0.3, vroughness=0.3, remaproughness=False)),
    ("glass_aniso", "glass", dict(Kr=(0.9, 0.9, 0.8), Kt=(0.8, 0.9, 0.9), eta=1.5, uroughness=0.2, vroughness=0.5, remaproughness=False)),
    ("glass_kr", "glass", dict(Kr=(0.9, 0.9, 0.8), Kt=(0.0, 0.0, 0.0), eta=1.5, uroughness=0.3, vroughness=0.3, remaproughness=False)),
    ("glass_kt", "glass", dict(Kr=(0.0, 0.0, 0.0), Kt=(0.8, 0.9, 0.9), eta=1.5, uroughness=0.8, vroughness=0.8, remaproughness=False)),
    ("glass_eta11", "glass", dict(eta=1.1, uroughness=0.3, vroughness=0.3, remaproughness=False)),
    ("glass_eta_inv", "glass", dict(eta=1.0 / 1.5, uroughness=0.3, vroughness=0.3, remaproughness=False)),
    ("glass_specular", "glass", dict(Kr=(0.9, 0.9, 0.8), Kt=(0.8, 0.9, 0.9), eta=1.5, uroughness=0.0, vroughness=0.0, remaproughness=False)),
]
# edge configurations of the device comparison only: the value properties exclude eta == 1 (sqrt_denom is 0 there)
EDGE_CONFIGS = [
    ("glass_eta1_rough", "glass", dict(eta=1.0, uroughness=0.3, vroughness=0.3, remaproughness=False)),
    ("glass_eta1_specular", "glass", dict(eta=1.0, uroughness=0.0, vroughness=0.0, remaproughness=False)),
    ("glass_remap", "glass", dict(eta=1.5, uroughness=0.0, vroughness=0.2, remaproughness=True)),
]
BY_NAME = {c[0]: c for c in CONFIGS + EDGE_CONFIGS}

# ---- measured tolerances.  Metric: |got - want| / max(|want|, FLOOR) per component over f, pdf and the sample's f, wi, pdf,
# rows flagged fragile by the restatement left out.  Measured with the libm oracle against the binary64 restatement on the CPU over
# every configuration and flag set of test_oracle_matches_the_restatement: 99.9th percentile MEASURED_P999, maximum MEASURED_MAX.  The
# bounds are 4 x the measurement: the deterministic math is within 1 ulp of libm in tan / atan / sin / cos, and rounding differs per input set.
FLOOR = 1.0e-3
MEASURED_P999, MEASURED_MAX = 1.17e-4, 1.67e-2      # metal_aniso_vu (anisotropic sample_wh) / the matte family (a cosine-sampled wi.z of 1e-3)
TOL_P999, TOL_MAX = 4.0 * MEASURED_P999, 4.0 * MEASURED_MAX
MEASURED_FRAGILE_SHARE = 0.0004             # largest share of rows left out in one (configuration, flag set) of that test, libm oracle
MAX_FRAGILE_SHARE = 0.005


class Hook:
    """the BSDF hook of one backend over one scene that holds every configuration"""

    def __init__(self, be, configs=None):
        self.be = be
        b = SceneBuilder(be)
        self.index = {}
        for name, kind, params in (configs or CONFIGS + EDGE_CONFIGS):
            self.index[name] = b.material(kind, **params)
        b.shape("sphere")
        self.scene = b.create_scene()
        self.fn = be.lib.orc_test_bsdf if be.is_oracle else be.lib.ftn_test_bsdf
        self.fn.argtypes = A.TEST_BSDF_ARGTYPES
        self.fn.restype = C.c_int

    def raw(self, name, flags, aml, rows, specialised=0):
        mat = self.index[name]
        return run_rows(self.be, lambda pin, n, pout: self.fn(self.scene.handle, mat, flags, int(aml), int(specialised), pin, n, pout),
                        rows, A.FTN_TEST_BSDF_IN, A.FTN_TEST_BSDF_OUT)

    def __call__(self, name, flags, aml, rows, specialised=0):
        return R.unpack(self.raw(name, flags, aml, rows, specialised))


def check_refuses_textured_materials(be):
    """a material with a textured parameter is resolved per hit, which is not this hook's business: FTN_ERR_UNSUPPORTED and nothing written, while
    a constant material of the same scene is still served"""
    b = SceneBuilder(be)
    b.texture("chk", "spectrum", "checkerboard", tex1=(0.1, 0.2, 0.3), tex2=(0.8, 0.7, 0.6))
    b.texture("fchk", "float", "checkerboard", tex1=0.0, tex2=30.0)
    mats = [b.material("matte", Kd="chk"), b.material("matte", Kd=(0.5, 0.4, 0.3), sigma="fchk"), b.material("plastic", Ks="chk"),
            b.material("matte", Kd=(0.5, 0.4, 0.3))]
    b.shape("sphere")
    scene = b.create_scene()
    fn = be.lib.orc_test_bsdf if be.is_oracle else be.lib.ftn_test_bsdf
    fn.argtypes = A.TEST_BSDF_ARGTYPES
    fn.restype = C.c_int
    rows = random_rows(3, 8)
    for k, mat in enumerate(mats):
        out = np.full((8, A.FTN_TEST_BSDF_OUT), 7.0, f32)
        rc = fn(scene.handle, mat, ALL, 0, 0, rows.ctypes.data_as(C.c_void_p), 8, out.ctypes.data_as(C.c_void_p))
        if k < 3:
            assert rc == A.FTN_ERR_UNSUPPORTED and np.all(out == 7.0), (k, rc)
        else:
            assert rc == A.FTN_OK and np.all(out[:, 0] == 1.0) and np.all(out[:, 1] == 1.0), (k, rc)


# ---------------------------------------------------------------- rows
def unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def frames(rng, n, general):
    """ng, ns, dpdu.  general: ns up to 80 degrees from ng, dpdu neither unit nor orthogonal to ns; else an orthonormal frame with ns == ng"""
    ng = unit(rng, n)
    t = np.cross(ng, unit(rng, n)); t /= np.linalg.norm(t, axis=1, keepdims=True)
    if not general:
        return ng, ng.copy(), t
    ang = np.radians(rng.uniform(0.0, 80.0, n))[:, None]
    ns = np.cos(ang) * ng + np.sin(ang) * t
    t2 = np.cross(ns, unit(rng, n)); t2 /= np.linalg.norm(t2, axis=1, keepdims=True)
    dpdu = (t2 + rng.uniform(-0.5, 0.5, n)[:, None] * ns) * np.exp(rng.uniform(np.log(0.1), np.log(10.0), n))[:, None]
    return ng, ns, dpdu


def random_rows(seed, n, general=True, margin=0.02):
    """(wo, wi, u) dense on the whole sphere with random frames, kept `margin` away from the hemisphere tests on ng and ns and from the
    lobe choice at u.x = 1/2"""
    rng = np.random.default_rng(seed)
    m = int(n * 1.6) + 64
    ng, ns, dpdu = frames(rng, m, general)
    wo, wi = unit(rng, m), unit(rng, m)
    u = rng.random((m, 2))
    rows = np.concatenate([ng, ns, dpdu, wo, wi, u], axis=1).astype(f32)
    r = rows.astype(np.float64)
    keep = np.ones(m, bool)
    for w in (r[:, 9:12], r[:, 12:15]):
        keep &= (np.abs(R.dot(w, r[:, 0:3])) >= margin) & (np.abs(R.dot(w, r[:, 3:6])) >= margin)
    keep &= (r[:, 15] < 1.0) & (r[:, 16] < 1.0)
    if margin > 0.0:
        keep &= np.abs(r[:, 15] - 0.5) >= 1.0e-3
    rows = rows[keep]
    assert rows.shape[0] >= n
    return rows[:n]


def local_rows(wo, wi, u):
    """rows in the identity frame (ng = ns = +z, dpdu = +x): world and local coordinates coincide exactly"""
    wo, wi, u = np.atleast_2d(wo), np.atleast_2d(wi), np.atleast_2d(u)
    n = max(len(wo), len(wi), len(u))
    rows = np.zeros((n, 17), f32)
    rows[:, 2] = 1.0; rows[:, 5] = 1.0; rows[:, 6] = 1.0
    rows[:, 9:12] = wo; rows[:, 12:15] = wi; rows[:, 15:17] = u
    return rows


def direction(theta_deg, phi=0.3):
    t = np.radians(theta_deg)
    return np.array([np.sin(t) * np.cos(phi), np.sin(t) * np.sin(phi), np.cos(t)])


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(all="ignore"):
        e = np.abs(got - want) / np.maximum(np.abs(want), FLOOR)
    both_nan = np.isnan(got) & np.isnan(want)
    both_inf = np.isinf(got) & (got == want)
    return np.where(both_nan | both_inf, 0.0, e)


def compare_with_restatement(hook, name, flags, aml, rows, **kw):
    """-> (errors over the compared values, share of rows left out).  Asserts the discrete outcomes on the rows that are compared."""
    _, kind, params = BY_NAME[name]
    want = R.evaluate(kind, params, flags, aml, rows, **kw)
    got = hook(name, flags, aml, rows)
    assert np.all(got["accepted"] == (1.0 if want["accepted"] else 0.0)), name
    if not want["accepted"]:
        return np.zeros(0), 0.0
    assert np.all(got["n_lobes"] == want["n_lobes"]), name
    ok = ~want["fragile"]
    assert np.array_equal(got["s_ok"][ok], want["s_ok"][ok]), (name, flags)
    assert np.array_equal(got["s_type"][ok], want["s_type"][ok]), (name, flags)
    s = ok & want["s_ok"]
    errs = [rel_err(got["f"][ok], want["f"][ok]).ravel(), rel_err(got["pdf"][ok], want["pdf"][ok]),
            rel_err(got["s_f"][s], want["s_f"][s]).ravel(), rel_err(got["s_wi"][s], want["s_wi"][s]).ravel(), rel_err(got["s_pdf"][s], want["s_pdf"][s])]
    return np.concatenate(errs), 1.0 - ok.mean()


def check_signed_zeros(hook, name, n=4000, seed=16):
    """wo.z and wi.z at +0 and -0 in the identity frame: same_hemisphere (reflection/mod.rs:84-86) goes by the sign bit, so +0 is the upper side
    and -0 the lower one; a sample from wo.z == +-0 is still drawn (only f and pdf return early, bsdf.rs:70, :134).  Outcomes and values
    against the restatement, the zeros themselves not counted as fragile."""
    rng = np.random.default_rng(seed)
    zero = [np.array([np.cos(a), np.sin(a), z]) for a, z in ((0.3, 0.0), (0.3, -0.0), (2.0, 0.0), (2.0, -0.0))]
    wos = zero + [direction(40.0), direction(140.0)]
    wis = zero + [direction(50.0, 2.0), direction(130.0, 2.0)]
    pairs = [(a, b) for a in wos for b in wis]
    k = n // len(pairs) + 1
    wo = np.repeat(np.array([p[0] for p in pairs]), k, axis=0)
    wi = np.repeat(np.array([p[1] for p in pairs]), k, axis=0)
    rows = local_rows(wo, wi, rng.random((len(wo), 2)))
    assert np.signbit(rows[:, 11]).any() and (rows[:, 11] == 0.0).any()
    for flags in (ALL, NON_SPECULAR):
        err, left_out = compare_with_restatement(hook, name, flags, 0, rows, exact_zero_is_firm=True)
        assert left_out <= 0.02, (name, left_out)                         # the sampled directions of wo.z == 0 hug the horizon more often
        assert err.size and err.max() <= TOL_MAX, (name, err.max())


# ---------------------------------------------------------------- properties (no one's reading of the reference involved)
def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def check_sample_eval_consistency(hook, name, n=200000, seed=11):
    """f(wo, s.wi) and pdf(wo, s.wi) reproduce an accepted non-specular sample's f and pdf: bit for bit, except the pdf of a sample drawn
    from a microfacet reflection lobe, which keeps the sampled wh where pdf() renormalises wo + wi (TOL_MAX there)."""
    rng = np.random.default_rng(seed)
    wo = unit(rng, n)
    wo = wo[np.abs(wo[:, 2]) >= 0.02]
    u = rng.random((len(wo), 2)).astype(f32)
    s = hook(name, ALL, 0, local_rows(wo, [0.0, 0.0, 1.0], u))
    take = s["s_ok"] & ((s["s_type"] & A.BSDF_SPECULAR) == 0)
    if not take.any():
        return 0
    e = hook(name, ALL, 0, local_rows(wo[take], s["s_wi"][take], u[take]))
    assert np.array_equal(bits(e["f"]), bits(s["s_f"][take])), name
    own_wh = s["s_type"][take] == (A.BSDF_REFLECTION | A.BSDF_GLOSSY)
    assert np.array_equal(bits(e["pdf"][~own_wh]), bits(s["s_pdf"][take][~own_wh])), name
    if own_wh.any():
        err = rel_err(e["pdf"][own_wh], s["s_pdf"][take][own_wh])
        assert err.max() <= TOL_MAX, (name, err.max())
    return int(take.sum())


RECIPROCAL = ["matte_lambert", "matte_sigma20", "matte_sigma90", "matte_negative", "plastic_kd", "plastic_ks", "plastic_both", "plastic_both_noremap",
              "metal_iso", "metal_iso_remap", "metal_aniso_uv", "metal_aniso_vu", "glass_kr", "glass_rough"]
# f(wo, wi) and f(wi, wo) share wh = wi + wo bit for bit; what differs is the order of the two lambdas in G (1 ulp), the Fresnel argument
# dot(wi, wh) against dot(wo, wh) (equal in exact arithmetic, 3 roundings of 2^-24 each here) and the order of the cosines in the
# denominator: a few 1e-7 relative, times the Fresnel term's sensitivity to its cosine (at most 1 / 0.05 with the cosines kept >= 0.05)
RECIPROCITY_TOL = 1.0e-4


def check_reciprocity(hook, name, n=100000, seed=12):
    rng = np.random.default_rng(seed)
    wo, wi = unit(rng, n), unit(rng, n)
    keep = (np.abs(wo[:, 2]) >= 0.05) & (np.abs(wi[:, 2]) >= 0.05) & (wo[:, 2] * wi[:, 2] > 0)       # reflection lobes only: transmission (radiance mode) is not reciprocal
    # the dielectric Fresnel term has a square-root singularity at the critical angle (cos_theta_t = sqrt(1 - sin2_theta_t), fresnel.rs:16): a
    # rounding of 1e-7 in its cosine moves it by sqrt(1e-7) there.  Every dielectric here has the ratio 1.5; pairs whose half-angle cosine
    # c = dot(wo, wh) comes within 1e-2 of 1 - 2.25 (1 - c^2) = 0 are left out (for all configurations alike: it costs 1 % of the pairs)
    wh = R.normalize(wo + wi)
    c = R.dot(wo, wh)
    keep &= np.abs(1.0 - 2.25 * (1.0 - c * c)) >= 1.0e-2
    wo, wi = wo[keep], wi[keep]
    flags = A.BSDF_REFLECTION | A.BSDF_DIFFUSE | A.BSDF_GLOSSY
    a = hook(name, flags, 0, local_rows(wo, wi, [0.5, 0.5]))["f"].astype(np.float64)
    b = hook(name, flags, 0, local_rows(wi, wo, [0.5, 0.5]))["f"].astype(np.float64)
    assert np.all(np.isfinite(a)) and a.max() > 0.0, name
    err = np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1.0e-6)
    assert err.max() <= RECIPROCITY_TOL, (name, err.max())


def check_sanity(hook, name, n=200000, seed=13):
    """f >= 0, pdf >= 0, everything finite, |wo.z| and |wi.z| >= 1e-3 (orthonormal frames, shading normal == geometric normal or not)"""
    rng = np.random.default_rng(seed)
    rows = random_rows(seed, n, general=False, margin=1.0e-3)
    half = n // 2                                     # second half: tilt the geometric normal away from the shading frame
    rows[half:, 0:3] = unit(rng, n - half).astype(f32)
    for flags in (ALL, NON_SPECULAR):
        o = hook(name, flags, 0, rows)
        for key in ("f", "pdf"):
            assert np.all(np.isfinite(o[key])) and np.all(o[key] >= 0.0), (name, key)
        s = o["s_ok"]
        for key in ("s_f", "s_pdf", "s_wi"):
            assert np.all(np.isfinite(o[key][s])), (name, key)
        assert np.all(o["s_f"][s] >= 0.0) and np.all(o["s_pdf"][s] > 0.0), name


# ---- histogram of sampled directions against the restatement's pdf
def wilson_hilferty(dof, p_tail):
    """the 1 - p_tail quantile of chi-square(dof): dof * (1 - 2/(9 dof) + z sqrt(2/(9 dof)))^3 with z the normal quantile (Acklam's rational
    approximation of the tail, relative error 1.2e-9)"""
    q = p_tail
    c = [-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00, -2.549732539343734e+00, 4.374664141464968e+00, 2.938163982698783e+00]
    d = [7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00]
    assert q < 0.02425
    t = np.sqrt(-2.0 * np.log(q))
    z = -(((((c[0] * t + c[1]) * t + c[2]) * t + c[3]) * t + c[4]) * t + c[5]) / ((((d[0] * t + d[1]) * t + d[2]) * t + d[3]) * t + 1.0)
    h = 2.0 / (9.0 * dof)
    return dof * (1.0 - h + z * np.sqrt(h)) ** 3


HIST_N = 4000000
# (configuration, theta_o in degrees): alpha >= 0.1 and theta_o <= 80 degrees, where the per-bin quadrature below converges (asserted)
HIST_CASES = [("matte_sigma20", 30), ("plastic_both", 0), ("plastic_both", 60), ("plastic_both_noremap", 80), ("plastic_ks", 30),
              ("metal_iso", 0), ("metal_iso", 30), ("metal_iso", 60), ("metal_iso", 80), ("glass_kr", 60),
              ("glass_kt", 0), ("glass_rough", 30), ("glass_aniso", 60), ("glass_eta_inv", 30)]


def expected_fractions(name, wo, two_sided, sub):
    """per bin: the integral of the restatement's pdf over the bin (sub x sub Gauss-Legendre points per bin) and whether the whole
    bin is reachable (transmitted directions: the generalised half vector separates wo and wi, mod.rs:408-427)"""
    _, kind, params = BY_NAME[name]
    lobes = R.material_lobes(kind, False, **params)
    nz, nphi = (20 if two_sided else 10), 20
    z0 = -1.0 if two_sided else 0.0
    # Gauss-Legendre nodes in (theta, phi) per bin, weight sin(theta): directions are smooth in theta up to the poles, where the midpoint rule in
    # cos(theta) meets a square-root singularity (it needed more than 64 x 64 points per bin there)
    x, w = np.polynomial.legendre.leggauss(sub)
    edges = np.arccos(np.clip(z0 + (1.0 - z0) * np.arange(nz + 1) / nz, -1.0, 1.0))                 # decreasing theta
    tlo, thi = edges[1:], edges[:-1]
    th = (0.5 * (tlo + thi)[:, None] + 0.5 * (thi - tlo)[:, None] * x[None, :]).ravel()
    wth = (0.5 * (thi - tlo)[:, None] * w[None, :]).ravel() * np.sin(th)
    ps = (2.0 * np.pi / nphi * (np.arange(nphi)[:, None] + 0.5 + 0.5 * x[None, :])).ravel()
    wps = np.tile(np.pi / nphi * w, nphi)
    T, P = np.meshgrid(th, ps, indexing="ij")
    wi = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], axis=-1).reshape(-1, 3)
    wo_b = np.broadcast_to(wo, wi.shape)
    n = wi.shape[0]
    ident = R.Bsdf(lobes, np.broadcast_to([0.0, 0.0, 1.0], (n, 3)), np.broadcast_to([0.0, 0.0, 1.0], (n, 3)), np.broadcast_to([1.0, 0.0, 0.0], (n, 3)))
    pdf = ident.pdf(wo_b, wi, NON_SPECULAR)
    pdf = (pdf.reshape(nz * sub, nphi * sub) * wth[:, None] * wps[None, :]).reshape(nz, sub, nphi, sub)
    frac = pdf.sum(axis=(1, 3))
    # reachability on a lattice that includes the bins' borders (Gauss-Legendre nodes stay inside, and the rim of the reachable region may cut a corner)
    lat = np.linspace(0.0, 1.0, sub + 1)
    th = (thi[:, None] + (tlo - thi)[:, None] * lat[None, :]).ravel()
    ps = (2.0 * np.pi / nphi * (np.arange(nphi)[:, None] + lat[None, :])).ravel()
    T, P = np.meshgrid(th, ps, indexing="ij")
    wi = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], axis=-1).reshape(-1, 3)
    wo_b = np.broadcast_to(wo, wi.shape)
    reach = np.ones(wi.shape[0], bool)
    for l in lobes:
        if l.kind == "mf_t":
            reach &= (wi[:, 2] * wo[2] >= 0.0) | l.reachable(wo_b, wi)
    reach = reach.reshape(nz, sub + 1, nphi, sub + 1).all(axis=(1, 3))
    return frac.ravel(), reach.ravel()


def check_histogram(hook, name, theta_o, seed=14, sub=16):
    """-> (chi2, dof, quantile).  The sampled directions' histogram against N x the integral of pdf per bin (Pearson chi-square, 1 - 1e-7 quantile by
    Wilson-Hilferty) and the accepted fraction against the integral of pdf over the bins that take part (5 sigma binomial)."""
    _, kind, params = BY_NAME[name]
    two_sided = kind == "glass" and any(l.kind == "mf_t" for l in R.material_lobes(kind, False, **params))
    wo = direction(theta_o).astype(f32).astype(np.float64)
    frac, reach = expected_fractions(name, wo, two_sided, sub)
    frac2, reach2 = expected_fractions(name, wo, two_sided, 2 * sub)
    expect, expect2 = HIST_N * frac, HIST_N * frac2
    part = reach & reach2
    assert np.all(np.abs(expect2 - expect)[part] <= 0.1 * np.sqrt(expect2[part])), (name, theta_o, "the quadrature has not converged")
    rng = np.random.default_rng(seed)
    u = rng.random((HIST_N, 2)).astype(f32)
    s = hook(name, NON_SPECULAR, 0, local_rows(wo, [0.0, 0.0, 1.0], u))
    wi = s["s_wi"][s["s_ok"]].astype(np.float64)
    nz, nphi = (20 if two_sided else 10), 20
    z0 = -1.0 if two_sided else 0.0
    iz = np.clip(np.floor((wi[:, 2] - z0) / (1.0 - z0) * nz).astype(int), 0, nz - 1)
    ip = np.clip(np.floor(np.mod(np.arctan2(wi[:, 1], wi[:, 0]), 2.0 * np.pi) / (2.0 * np.pi) * nphi).astype(int), 0, nphi - 1)
    if not two_sided:
        assert np.all(wi[:, 2] >= 0.0), name
    counts = np.bincount(iz * nphi + ip, minlength=nz * nphi).astype(np.float64)
    big = part & (expect2 >= 5.0)
    small = part & ~big
    obs = list(counts[big]); exp = list(expect2[big])
    if expect2[small].sum() >= 5.0:                   # the bins below 5 expected samples, pooled
        obs.append(counts[small].sum()); exp.append(expect2[small].sum())
    obs, exp = np.array(obs), np.array(exp)
    # what is left over (rejected samples, samples outside the bins that take part) is one more cell
    rest_exp = HIST_N - exp.sum()
    rest_obs = HIST_N - obs.sum()
    chi2 = float(np.sum((obs - exp) ** 2 / exp))
    dof = len(exp)
    if rest_exp >= 5.0:
        chi2 += (rest_obs - rest_exp) ** 2 / rest_exp
    else:
        dof -= 1
    quant = float(wilson_hilferty(dof, 1.0e-7))
    print("histogram %-22s theta_o %2d: chi2 %.1f dof %d quantile %.1f z %.2f" % (name, theta_o, chi2, dof, quant, (chi2 - dof) / np.sqrt(2.0 * dof)))
    assert chi2 <= quant, (name, theta_o, chi2, dof, quant)
    p = frac2[part].sum()                              # integral of pdf over the participating bins == share of the samples that land there
    landed = counts[part].sum()
    sigma = np.sqrt(HIST_N * p * max(1.0 - p, 1.0e-12))
    assert abs(landed - HIST_N * p) <= 5.0 * sigma + 1.0, (name, theta_o, landed, HIST_N * p, sigma)
    return chi2, dof, quant


# ---- pinned reference quirks: (configuration, wo, unreachable wi, whether the generalised half vector separates wo and wi)
QUIRKS = [("glass_kt", np.array([0.0, 0.0, 1.0]), [direction(100.0, 0.0), direction(110.0, 1.0), direction(125.0, 2.0)], False),
          ("glass_aniso", direction(60.0), [direction(95.0, 4.0), direction(100.0, 3.5), direction(105.0, 4.0)], True)]


def check_quirk_pin(hook, name, wo, wis, separated):
    """pdf() of microfacet transmission is positive at fixed directions no sample reaches, with the restatement's value (test_bsdf_cpu.py names the
    two cases and the reference's lines)"""
    rows = local_rows(wo, np.array(wis), [0.5, 0.5])
    _, kind, params = BY_NAME[name]
    lobe = [l for l in R.material_lobes(kind, False, **params) if l.kind == "mf_t"][0]
    r = rows.astype(np.float64)
    wh, _ = lobe.generalised_half(r[:, 9:12], r[:, 12:15])
    assert not lobe.reachable(r[:, 9:12], r[:, 12:15]).any()
    assert np.all((R.dot(r[:, 9:12], wh) * R.dot(r[:, 12:15], wh) < 0.0) == separated)
    flags = A.BSDF_TRANSMISSION | A.BSDF_GLOSSY
    want = R.evaluate(kind, params, flags, 0, rows)["pdf"]
    got = hook(name, flags, 0, rows)["pdf"]
    assert np.all(want > 1.0e-3) and np.all(got > 0.0)
    assert rel_err(got, want).max() <= TOL_MAX
    # and no sample lands there: every transmitted sample is reachable in the sense above
    u = np.random.default_rng(15).random((200000, 2)).astype(f32)
    s = hook(name, flags, 0, local_rows(wo, wo, u))
    wi = s["s_wi"][s["s_ok"]].astype(np.float64)
    wo_b = np.broadcast_to(rows[0, 9:12].astype(np.float64), wi.shape)
    wh, _ = lobe.generalised_half(wo_b, wi)
    wh = np.where((wh[:, 2] < 0.0)[:, None], -wh, wh)
    assert len(wi) > 1000 and np.all(R.dot(wo_b, wh) * R.dot(wi, wh) < 1.0e-6) and np.all(R.dot(wo_b, wh) > -1.0e-6)
