"""An independent binary64 restatement of the reference's BSDF code, written from its Rust sources (cited per function as
file:lines under src/), vectorised over rows.  It takes what the BSDF hook takes (ftn_test_bsdf / orc_test_bsdf: rows of
ng, ns, dpdu, wo, wi, u and a material given by its SceneBuilder parameters) and returns the same outputs, so the oracle and the
device can be laid next to it.  Nothing here is derived from oracle/ or fountain_amd/csrc/.

Branch bookkeeping: every comparison the reference makes on a computed quantity (hemisphere tests, `sin2_theta_t >= 1`,
`floor(u.x * n)`, the geometric reflect / transmit choice) also records how close the quantity came to its threshold; `fragile`
marks rows where some distance is below `tol`, i.e. where binary32 rounding may legitimately take the other branch."""
import numpy as np

REFLECTION, TRANSMISSION, DIFFUSE, GLOSSY, SPECULAR, ALL = 1, 2, 4, 8, 16, 31      # reflection/mod.rs:14-22
ROW_IN, ROW_OUT = 17, 16

_f32 = np.float32


def _c(v):
    """a parameter as the binary32 value the libraries store, in binary64"""
    return np.asarray(v, _f32).astype(np.float64)


def dot(a, b):
    return np.sum(a * b, axis=-1)


def normalize(a):
    with np.errstate(all="ignore"):
        return a / np.sqrt(dot(a, a))[..., None]


def cross(a, b):
    return np.cross(a, b)


def sign_positive(x):                      # f32::is_sign_positive: the sign bit, so -0.0 is negative
    return ~np.signbit(x)


# ---------------------------------------------------------------- reflection/mod.rs:24-91
def cos2_theta(w): return w[..., 2] * w[..., 2]
def sin2_theta(w): return np.maximum(0.0, 1.0 - cos2_theta(w))
def sin_theta(w): return np.sqrt(sin2_theta(w))


def tan_theta(w):
    with np.errstate(all="ignore"):
        return sin_theta(w) / w[..., 2]


def tan2_theta(w):
    with np.errstate(all="ignore"):
        return sin2_theta(w) / cos2_theta(w)


def cos_phi(w):                            # :44-51
    s = sin_theta(w)
    with np.errstate(all="ignore"):
        return np.where(s == 0.0, 1.0, np.clip(w[..., 0] / s, -1.0, 1.0))


def sin_phi(w):                            # :53-60
    s = sin_theta(w)
    with np.errstate(all="ignore"):
        return np.where(s == 0.0, 0.0, np.clip(w[..., 1] / s, -1.0, 1.0))


def refract(wi, n, eta):                   # :70-78 -> (ok, wt, 1 - sin2_theta_t)
    ci = dot(n, wi)
    s2i = np.maximum(0.0, 1.0 - ci * ci)
    s2t = eta * eta * s2i
    ok = ~(s2t >= 1.0)
    with np.errstate(all="ignore"):
        ct = np.sqrt(1.0 - s2t)
    wt = np.asarray(eta)[..., None] * -wi + (eta * ci - ct)[..., None] * n
    return ok, wt, 1.0 - s2t


def reflect(wo, n):                        # :80-82
    return -wo + 2.0 * dot(wo, n)[..., None] * n


def same_hemisphere(a, b):                 # :84-86
    return sign_positive(a[..., 2]) == sign_positive(b[..., 2])


def faceforward(v1, v2):                   # geometry/mod.rs:64-70
    return np.where((dot(v1, v2) < 0.0)[..., None], -v1, v1)


# ---------------------------------------------------------------- fresnel.rs
def fresnel_dielectric(cos_i, eta_i, eta_t):           # :4-22
    ci = np.clip(cos_i, -1.0, 1.0)
    entering = ci > 0.0
    ei = np.where(entering, eta_i, eta_t)
    et = np.where(entering, eta_t, eta_i)
    ci = np.abs(ci)
    si = np.sqrt(np.maximum(1.0 - ci * ci, 0.0))
    st = ei / et * si
    ct = np.sqrt(np.maximum(1.0 - st * st, 0.0))
    with np.errstate(all="ignore"):
        rpar = ((et * ci) - (ei * ct)) / ((et * ci) + (ei * ct))
        rper = ((ei * ci) - (et * ct)) / ((ei * ci) + (et * ct))
    return np.where(st >= 1.0, 1.0, (rpar * rpar + rper * rper) / 2.0)


def fresnel_conductor(cos_i, eta_i, eta_t, k):         # :25-48; cos_i [N], spectra [3] -> [N, 3]
    ci = np.clip(cos_i, -1.0, 1.0)[..., None]
    eta, eta_k = eta_t / eta_i, k / eta_i
    c2 = ci * ci
    s2 = 1.0 - c2
    eta2, etak2 = eta * eta, eta_k * eta_k
    t0 = eta2 - etak2 - s2
    a2b2 = np.sqrt(t0 * t0 + 4.0 * eta2 * etak2)
    t1 = a2b2 + c2
    a = np.sqrt(0.5 * (a2b2 + t0))
    t2 = 2.0 * ci * a
    with np.errstate(all="ignore"):
        rs = (t1 - t2) / (t1 + t2)
        t3 = c2 * a2b2 + s2 * s2
        t4 = t2 * s2
        rp = rs * (t3 - t4) / (t3 + t4)
    return 0.5 * (rp + rs)


def fresnel_evaluate(fr, cos_i):                       # :69-103 -> [N, 3]
    if fr[0] == "dielectric":
        return np.repeat(fresnel_dielectric(cos_i, fr[1], fr[2])[..., None], 3, axis=-1)
    if fr[0] == "conductor":
        return fresnel_conductor(np.abs(cos_i), fr[1], fr[2], fr[3])
    return np.ones(cos_i.shape + (3,))


# ---------------------------------------------------------------- reflection/microfacet.rs
def roughness_to_alpha(roughness):                     # :40-45 (TrowbridgeReitz forwards to it, :125-127)
    x = np.log(np.maximum(roughness, _c(1.0e-3)))
    return _c(1.62142) + _c(0.819955) * x + _c(0.1734) * x * x + _c(0.0171201) * x * x * x + _c(0.000640711) * x * x * x * x


def tr_d(ax, ay, wh):                                  # :135-146
    t2 = tan2_theta(wh)
    c4 = cos2_theta(wh) * cos2_theta(wh)
    with np.errstate(all="ignore"):
        e = (cos_phi(wh) ** 2 / (ax * ax) + sin_phi(wh) ** 2 / (ay * ay)) * t2
        d = 1.0 / (np.pi * ax * ay * c4 * (1.0 + e) * (1.0 + e))
    return np.where(np.isinf(t2), 0.0, d)


def tr_lambda(ax, ay, w):                              # :148-160
    att = np.abs(tan_theta(w))
    alpha = np.sqrt(cos_phi(w) ** 2 * ax * ax + sin_phi(w) ** 2 * ay * ay)
    with np.errstate(all="ignore"):
        a2t2 = (alpha * att) * (alpha * att)
        lam = (-1.0 + np.sqrt(1.0 + a2t2)) / 2.0
    return np.where(np.isinf(att), 0.0, lam)


def tr_g(ax, ay, wo, wi):                              # :21-23
    return 1.0 / (1.0 + tr_lambda(ax, ay, wo) + tr_lambda(ax, ay, wi))


def tr_pdf(ax, ay, wh):                                # :28-31
    return tr_d(ax, ay, wh) * np.abs(wh[..., 2])


def tr_sample_wh(ax, ay, wo, u):                       # :162-186
    u0, u1 = u[..., 0], u[..., 1]
    with np.errstate(all="ignore"):
        if ax == ay:
            tt2 = (ax * ax) * u0 / (1.0 - u0)
            ct = 1.0 / np.sqrt(1.0 + tt2)
            phi = 2.0 * np.pi * u1
        else:
            phi = np.arctan(ay / ax * np.tan(2.0 * np.pi * u1 + 0.5 * np.pi))
            phi = np.where(u1 > 0.5, phi + np.pi, phi)
            sp, cp = np.sin(phi), np.cos(phi)
            alpha2 = 1.0 / ((cp * cp) / (ax * ax) + (sp * sp) / (ay * ay))
            tt2 = alpha2 * u0 / (1.0 - u0)
            ct = 1.0 / np.sqrt(1.0 + tt2)
    st = np.sqrt(np.maximum(0.0, 1.0 - ct * ct))
    wh = np.stack([st * np.cos(phi), st * np.sin(phi), ct], axis=-1)          # spherical_direction, math.rs:74-80
    return np.where(same_hemisphere(wo, wh)[..., None], wh, -wh)


# ---------------------------------------------------------------- sampling.rs:5-25
def concentric_sample_disk(u):
    ox, oy = 2.0 * u[..., 0] - 1.0, 2.0 * u[..., 1] - 1.0
    with np.errstate(all="ignore"):
        first = np.abs(ox) > np.abs(oy)
        theta = np.where(first, np.pi / 4 * (oy / ox), np.pi / 2 - np.pi / 4 * (ox / oy))
        r = np.where(first, ox, oy)
    zero = (ox == 0.0) & (oy == 0.0)
    theta = np.where(zero, 0.0, theta)
    r = np.where(zero, 0.0, r)
    return r * np.cos(theta), r * np.sin(theta)


def cosine_sample_hemisphere(u):
    x, y = concentric_sample_disk(u)
    return np.stack([x, y, np.sqrt(np.maximum(0.0, 1.0 - x * x - y * y))], axis=-1)


# ---------------------------------------------------------------- BxDFs: reflection/mod.rs:149-439
class Lobe:
    """kind: lambert | oren | spec_r | spec_t | mf_r | mf_t"""

    def __init__(self, kind, r, fresnel=("noop",), a=0.0, b=0.0, ax=0.0, ay=0.0, eta_a=1.0, eta_b=1.0):
        self.kind, self.r, self.fresnel, self.a, self.b, self.ax, self.ay, self.eta_a, self.eta_b = kind, np.asarray(r, np.float64), fresnel, a, b, ax, ay, eta_a, eta_b

    @property
    def type(self):
        return {"lambert": REFLECTION | DIFFUSE, "oren": REFLECTION | DIFFUSE, "spec_r": REFLECTION | SPECULAR,
                "spec_t": TRANSMISSION | SPECULAR, "mf_r": REFLECTION | GLOSSY, "mf_t": TRANSMISSION | GLOSSY}[self.kind]

    def matches(self, flags):                          # :98-100, t.contains(self.get_type())
        return (flags & self.type) == self.type

    def get_eta(self, wo):                             # :377-379
        return np.where(wo[..., 2] > 0.0, self.eta_b / self.eta_a, self.eta_a / self.eta_b)

    def generalised_half(self, wo, wi):                # the wh of :398 / :434, before any flip
        eta = self.get_eta(wo)
        return normalize(wo + wi * eta[..., None]), eta

    def reachable(self, wo, wi):
        """a transmitted pair (wo, wi) can only come from a microfacet whose normal has wo and wi on opposite sides (refract, :70-78), and
        sample_f drops a normal that faces away from wo once sample_wh has put it into wo's hemisphere (:412-415)"""
        wh, _ = self.generalised_half(wo, wi)
        wh = np.where((sign_positive(wh[..., 2]) != sign_positive(wo[..., 2]))[..., None], -wh, wh)
        return (dot(wo, wh) * dot(wi, wh) < 0.0) & (dot(wo, wh) >= 0.0)

    def f(self, wo, wi):
        n = wo.shape[:-1]
        k = self.kind
        if k == "lambert":                             # :159-161
            return np.broadcast_to(self.r / np.pi, n + (3,)).copy()
        if k == "oren":                                # :274-296
            sti, sto = sin_theta(wi), sin_theta(wo)
            d_cos = cos_phi(wi) * cos_phi(wo) + sin_phi(wi) * sin_phi(wo)
            max_cos = np.where((sti > 1.0e-4) & (sto > 1.0e-4), np.maximum(0.0, d_cos), 0.0)
            aci, aco = np.abs(wi[..., 2]), np.abs(wo[..., 2])
            with np.errstate(all="ignore"):
                first = aci > aco
                sin_alpha = np.where(first, sto, sti)
                tan_beta = np.where(first, sti / aci, sto / aco)
                return self.r / np.pi * (self.a + (self.b * max_cos * sin_alpha * tan_beta))[..., None]
        if k in ("spec_r", "spec_t"):                  # :181-183, :221-223
            return np.zeros(n + (3,))
        if k == "mf_r":                                # :318-336
            co, ci = np.abs(wo[..., 2]), np.abs(wi[..., 2])
            wh = wi + wo
            degenerate = (ci == 0.0) | (co == 0.0) | np.all(wh == 0.0, axis=-1)
            wh = normalize(wh)
            up = np.zeros_like(wh); up[..., 2] = 1.0
            fr = fresnel_evaluate(self.fresnel, dot(wi, faceforward(wh, up)))
            with np.errstate(all="ignore"):
                v = self.r * (tr_d(self.ax, self.ay, wh) * tr_g(self.ax, self.ay, wo, wi))[..., None] * fr / (4.0 * ci * co)[..., None]
            return np.where(degenerate[..., None], 0.0, v)
        # mf_t :387-406, TransportMode::Radiance
        co, ci = wo[..., 2], wi[..., 2]
        zero = same_hemisphere(wo, wi) | (co == 0.0) | (ci == 0.0)
        wh, eta = self.generalised_half(wo, wi)
        wh = np.where((wh[..., 2] < 0.0)[..., None], -wh, wh)
        fr = fresnel_evaluate(self.fresnel, dot(wo, wh))
        sqrt_denom = dot(wo, wh) + eta * dot(wi, wh)
        factor = 1.0 / eta
        with np.errstate(all="ignore"):
            s = np.abs(tr_d(self.ax, self.ay, wh) * tr_g(self.ax, self.ay, wo, wi) * eta * eta * np.abs(dot(wi, wh)) * np.abs(dot(wo, wh)) * factor * factor
                       / (ci * co * sqrt_denom * sqrt_denom))
            v = (1.0 - fr) * self.r * s[..., None]
        return np.where(zero[..., None], 0.0, v)

    def pdf(self, wo, wi):
        k = self.kind
        if k in ("lambert", "oren"):                   # :140-146
            return np.where(same_hemisphere(wo, wi), np.abs(wi[..., 2]) / np.pi, 0.0)
        if k in ("spec_r", "spec_t"):                  # :194-196, :246-248
            return np.zeros(wo.shape[:-1])
        if k == "mf_r":                                # :354-360
            wh = normalize(wo + wi)
            with np.errstate(all="ignore"):
                v = tr_pdf(self.ax, self.ay, wh) / (4.0 * dot(wo, wh))
            return np.where(same_hemisphere(wo, wi), v, 0.0)
        wh, eta = self.generalised_half(wo, wi)        # :429-438
        sqrt_denom = dot(wo, wh) + eta * dot(wi, wh)
        with np.errstate(all="ignore"):
            dwh_dwi = np.abs((eta * eta * dot(wi, wh)) / (sqrt_denom * sqrt_denom))
            v = tr_pdf(self.ax, self.ay, wh) * dwh_dwi
        return np.where(same_hemisphere(wo, wi), 0.0, v)

    def sample_f(self, wo, u):
        """-> ok [N], f [N, 3], wi [N, 3], pdf [N], distances to the branches taken [list of [N]]"""
        n = wo.shape[:-1]
        k = self.kind
        if k in ("lambert", "oren"):                   # :131-138
            wi = cosine_sample_hemisphere(u)
            wi[..., 2] = np.where(wo[..., 2] < 0.0, -wi[..., 2], wi[..., 2])
            return np.ones(n, bool), self.f(wo, wi), wi, self.pdf(wo, wi), [np.abs(wi[..., 2])]
        if k == "spec_r":                              # :185-192
            wi = wo * np.array([-1.0, -1.0, 1.0])
            with np.errstate(all="ignore"):
                f = fresnel_evaluate(self.fresnel, wi[..., 2]) * self.r / np.abs(wi[..., 2])[..., None]
            return np.ones(n, bool), f, wi, np.ones(n), []
        if k == "spec_t":                              # :225-244
            entering = wo[..., 2] > 0.0
            eta_i = np.where(entering, self.eta_a, self.eta_b)
            eta_t = np.where(entering, self.eta_b, self.eta_a)
            nrm = np.zeros_like(wo); nrm[..., 2] = 1.0
            nrm = np.where((dot(nrm, wo) < 0.0)[..., None], -nrm, nrm)          # Normal3::faceforward, geometry/mod.rs:144-150
            ok, wi, margin = refract(wo, nrm, eta_i / eta_t)
            with np.errstate(all="ignore"):
                ft = self.r * (1.0 - fresnel_evaluate(self.fresnel, wi[..., 2]))
                f = ft / np.abs(wi[..., 2])[..., None]
            return ok, f, wi, np.ones(n), [np.abs(margin)]
        if k == "mf_r":                                # :338-352
            wh = tr_sample_wh(self.ax, self.ay, wo, u)
            wi = reflect(wo, wh)
            ok = same_hemisphere(wo, wi)
            with np.errstate(all="ignore"):
                pdf = tr_pdf(self.ax, self.ay, wh) / (4.0 * dot(wo, wh))
            return ok, self.f(wo, wi), wi, pdf, [np.abs(wi[..., 2])]
        ok0 = ~(wo[..., 2] == 0.0)                     # mf_t :408-427
        wh = tr_sample_wh(self.ax, self.ay, wo, u)
        owh = dot(wo, wh)
        ok1 = ~(owh < 0.0)
        eta = self.get_eta(-wo)                        # "this inverts the eta fraction", :416
        ok2, wi, margin = refract(wo, wh, eta)
        wi = np.where(ok2[..., None], wi, np.array([0.0, 0.0, 1.0]))
        return ok0 & ok1 & ok2, self.f(wo, wi), wi, self.pdf(wo, wi), [np.abs(owh), np.abs(margin), np.abs(wi[..., 2])]


# ---------------------------------------------------------------- materials: material/*.rs
def material_lobes(kind, allow_multiple_lobes=False, **kw):
    """The BxDFs Material::compute_scattering_functions adds for constant parameters (the SceneBuilder.material keywords and defaults,
    loaders/constructors.rs:192-236), or None where the reference panics (glass.rs:66-67)."""
    clamp_positive = lambda s: np.maximum(s, 0.0)      # spectrum/mod.rs:96-98
    black = lambda s: bool(np.all(s == 0.0))           # spectrum/mod.rs:76-78
    remap = kw.get("remaproughness", True)
    lobes = []
    if kind == "matte":                                # matte.rs:36-52
        r = clamp_positive(_c(kw.get("Kd", (0.5, 0.5, 0.5))))
        sigma = np.clip(_c(kw.get("sigma", 0.0)), 0.0, 90.0)
        if not black(r):
            if sigma == 0.0:
                lobes.append(Lobe("lambert", r))
            else:                                      # OrenNayar::new(r, Deg(sigma)), reflection/mod.rs:260-266
                s2 = np.radians(sigma) ** 2
                lobes.append(Lobe("oren", r, a=1.0 - (s2 / (2.0 * (s2 + _c(0.33)))), b=_c(0.45) * s2 / (s2 + _c(0.09))))
    elif kind == "mirror":                             # mirror.rs:22-30
        r = clamp_positive(_c(kw.get("Kr", (0.9, 0.9, 0.9))))
        if not black(r):
            lobes.append(Lobe("spec_r", r))
    elif kind == "plastic":                            # plastic.rs:25-48 (no clamp_positive here)
        kd, ks = _c(kw.get("Kd", (0.25, 0.25, 0.25))), _c(kw.get("Ks", (0.25, 0.25, 0.25)))
        if not black(kd):
            lobes.append(Lobe("lambert", kd))
        if not black(ks):
            rough = _c(kw.get("roughness", 0.1))
            if remap:
                rough = roughness_to_alpha(rough)
            lobes.append(Lobe("mf_r", ks, fresnel=("dielectric", 1.5, 1.0), ax=rough, ay=rough))
    elif kind == "metal":                              # metal.rs:38-65
        rough = kw.get("roughness", 0.01)
        u, v = kw.get("uroughness"), kw.get("vroughness")
        if u is None or v is None:
            u = v = rough
        u, v = _c(u), _c(v)
        if remap:
            u, v = roughness_to_alpha(u), roughness_to_alpha(v)
        lobes.append(Lobe("mf_r", np.ones(3), fresnel=("conductor", np.ones(3), _c(kw["eta"]), _c(kw["k"])), ax=u, ay=v))
    elif kind == "glass":                              # glass.rs:52-93
        eta = _c(kw.get("eta", 1.5))
        r, t = clamp_positive(_c(kw.get("Kr", (1, 1, 1)))), clamp_positive(_c(kw.get("Kt", (1, 1, 1))))
        u, v = _c(kw.get("uroughness", 0.0)), _c(kw.get("vroughness", 0.0))
        if remap:
            u, v = roughness_to_alpha(u), roughness_to_alpha(v)
        specular = u == 0.0 and v == 0.0
        if specular and allow_multiple_lobes:
            return None
        fr = ("dielectric", 1.0, eta)
        if not black(r):
            lobes.append(Lobe("spec_r", r, fresnel=fr) if specular else Lobe("mf_r", r, fresnel=fr, ax=u, ay=v))
        if not black(t):
            lobes.append(Lobe("spec_t", t, fresnel=fr, eta_a=1.0, eta_b=eta) if specular else Lobe("mf_t", t, fresnel=fr, ax=u, ay=v, eta_a=1.0, eta_b=eta))
    else:
        raise ValueError(kind)
    return lobes


# ---------------------------------------------------------------- Bsdf: reflection/bsdf.rs
class Bsdf:
    def __init__(self, lobes, ng, ns, dpdu):           # :31-46
        self.lobes = lobes
        self.ng, self.ns = ng, ns
        self.ss = normalize(dpdu)
        self.ts = normalize(cross(ns, self.ss))

    def num_components(self, flags):                   # :52-54
        return sum(1 for l in self.lobes if l.matches(flags))

    def world_to_local(self, v):                       # :56-58
        return np.stack([dot(v, self.ss), dot(v, self.ts), dot(v, self.ns)], axis=-1)

    def local_to_world(self, v):                       # :60-65
        return self.ss * v[..., 0:1] + self.ts * v[..., 1:2] + self.ns * v[..., 2:3]

    def _sum_f(self, wo, wi, refl, flags):
        total = np.zeros(wo.shape)
        for l in self.lobes:
            if not l.matches(flags):
                continue
            use = refl if l.type & REFLECTION else ~refl               # every BxDF here is either a reflection or a transmission
            total = total + np.where(use[..., None], l.f(wo, wi), 0.0)
        return total

    def f(self, wo_w, wi_w, flags, margins=None):      # :67-82
        wi, wo = self.world_to_local(wi_w), self.world_to_local(wo_w)
        gi, go = dot(wi_w, self.ng), dot(wo_w, self.ng)
        refl = gi * go > 0.0
        if margins is not None:
            margins += [np.abs(wo[..., 2]), np.abs(wi[..., 2]), np.abs(gi), np.abs(go)]
        return np.where((wo[..., 2] == 0.0)[..., None], 0.0, self._sum_f(wo, wi, refl, flags))

    def pdf(self, wo_w, wi_w, flags):                  # :131-144
        wo, wi = self.world_to_local(wo_w), self.world_to_local(wi_w)
        n = self.num_components(flags)
        total = np.zeros(wo.shape[:-1])
        for l in self.lobes:
            if l.matches(flags):
                total = total + l.pdf(wo, wi)
        if n == 0:
            return np.zeros(wo.shape[:-1])
        return np.where(wo[..., 2] == 0.0, 0.0, total / n)

    def sample_f(self, wo_w, u, flags, margins=None):  # :85-129 -> ok, f, wi_world, pdf, sampled_type
        n_rows = wo_w.shape[:-1]
        matching = [l for l in self.lobes if l.matches(flags)]
        mc = float(len(matching))
        ok = np.zeros(n_rows, bool); f = np.zeros(n_rows + (3,)); wi_w = np.zeros(n_rows + (3,)); pdf = np.zeros(n_rows); typ = np.zeros(n_rows, np.int64)
        if mc == 0.0:
            return ok, f, wi_w, pdf, typ
        x = u[..., 0] * mc
        comp = np.minimum(np.floor(x), mc - 1.0)
        if margins is not None and mc > 1.0:
            margins.append(np.abs(x - np.round(x)))
        ur = np.stack([x - comp, u[..., 1]], axis=-1)
        wo = self.world_to_local(wo_w)
        go = dot(wo_w, self.ng)
        for k, lobe in enumerate(matching):
            sel = comp == k
            s_ok, s_f, s_wi, s_pdf, s_m = lobe.sample_f(wo, ur)
            with np.errstate(all="ignore"):
                s_ok = s_ok & ~(s_pdf == 0.0)
                wiw = self.local_to_world(s_wi)
                specular = bool(lobe.type & SPECULAR)
                if not specular and mc > 1.0:
                    for other in matching:
                        if other is not lobe:
                            s_pdf = s_pdf + other.pdf(wo, s_wi)
                if mc > 1.0:
                    s_pdf = s_pdf / mc
                gi = dot(wiw, self.ng)
                if not specular:
                    s_f = self._sum_f(wo, s_wi, gi * go > 0.0, flags)
            if margins is not None:
                big = np.full(n_rows, np.inf)
                margins += [np.where(sel, m, big) for m in s_m]
                if not specular:
                    margins.append(np.where(sel & s_ok, np.abs(gi), big))
            put = sel & s_ok
            ok |= put
            f = np.where(put[..., None], s_f, f); wi_w = np.where(put[..., None], wiw, wi_w); pdf = np.where(put, s_pdf, pdf); typ = np.where(put, lobe.type, typ)
        return ok, f, wi_w, pdf, typ


def evaluate(kind, params, flags, allow_multiple_lobes, rows, tol=1.0e-4, exact_zero_is_firm=False):
    """What the hook returns for these rows, in binary64: dict of accepted, n_lobes, f, pdf, s_ok, s_f, s_wi, s_pdf, s_type, fragile.
    exact_zero_is_firm: a branch quantity that is exactly 0 does not make its row fragile (for rows in the identity frame with z = +-0, where
    the local z is the input's z in any precision and the branch is decided by its sign bit)."""
    rows = np.asarray(rows, _f32).astype(np.float64).reshape(-1, ROW_IN)
    n = rows.shape[0]
    lobes = material_lobes(kind, allow_multiple_lobes, **params)
    out = dict(accepted=lobes is not None, n_lobes=0, f=np.zeros((n, 3)), pdf=np.zeros(n), s_ok=np.zeros(n, bool), s_f=np.zeros((n, 3)),
               s_wi=np.zeros((n, 3)), s_pdf=np.zeros(n), s_type=np.zeros(n, np.int64), fragile=np.zeros(n, bool))
    if lobes is None:
        return out
    b = Bsdf(lobes, rows[:, 0:3], rows[:, 3:6], rows[:, 6:9])
    wo, wi, u = rows[:, 9:12], rows[:, 12:15], rows[:, 15:17]
    margins = []
    out["n_lobes"] = b.num_components(flags)
    out["f"] = b.f(wo, wi, flags, margins)
    out["pdf"] = b.pdf(wo, wi, flags)
    out["s_ok"], out["s_f"], out["s_wi"], out["s_pdf"], out["s_type"] = b.sample_f(wo, u, flags, margins)
    frag = np.zeros(n, bool)
    for m in margins:
        frag |= ~(m >= tol) & ~((m == 0.0) & exact_zero_is_firm)             # NaN counts as fragile
    out["fragile"] = frag
    return out


def unpack(rows_out):
    """a hook's output rows as the same dict (binary32 values)"""
    o = np.asarray(rows_out, _f32).reshape(-1, ROW_OUT)
    return dict(accepted=o[:, 0], n_lobes=o[:, 1], f=o[:, 2:5], pdf=o[:, 5], s_ok=o[:, 6] != 0, s_f=o[:, 7:10], s_wi=o[:, 10:13], s_pdf=o[:, 13],
                s_type=o[:, 14].astype(np.int64))
