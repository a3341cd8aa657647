"""What the traversal tests hold a library to, with no walk and no build of its own.

Layer A, check_tree / check_lights: invariants of a flattened BVH (bvh.rs:27-158) and of Scene::lights (scene/mod.rs:32-49) that follow from the
builder's data alone; every comparison is exact.

Layer B, judge / check_closest / check_occluded / check_seams: every ray against every primitive in binary64 (the hit tests of _light_ref, the sphere's margins of _integrator_ref), each
pair a firm hit, a firm miss or doubtful, and the two-sided rules a library's t, primitive and occlusion must meet on every row."""
import functools

import numpy as np

import _integrator_ref as IG
import _traversal_common as C

F32 = np.float32


# ------------------------------------------------------------------ layer A
def centroids(lo, hi):
    """Bounds3::centroid (bounds.rs:161-163): min + (max - min) / 2, in binary32"""
    return (lo + (hi - lo) / F32(2.0)).astype(F32)


def max_extent(lo, hi):                               # bounds.rs:169-178
    d = (hi - lo).astype(F32)
    return 0 if (d[0] > d[1] and d[0] > d[2]) else (1 if d[1] > d[2] else 2)


def check_tree(builder, nodes, order, depth):
    """nodes: NODE_DTYPE records; order: BVH index -> the builder's index; depth: what the library reports"""
    plo, phi = C.prim_bounds(builder)
    n = len(plo)
    order = np.asarray(order, np.int64)
    assert len(order) == n and np.array_equal(np.sort(order), np.arange(n)), "order is no permutation of the builder's primitives"
    if n == 0:
        assert len(nodes) == 0
        return dict(leaves=0, interior=0, depth=0, widest_leaf=0, fallbacks=0)
    lo, hi = plo[order], phi[order]                   # in BVH order
    cen = centroids(lo, hi)
    seen = np.zeros(len(nodes), np.int64)
    stats = dict(leaves=0, interior=0, depth=0, widest_leaf=0, fallbacks=0)
    next_prim = [0]

    def visit(i, level):
        """-> (one past the subtree's last node, first primitive, one past its last primitive)"""
        assert 0 <= i < len(nodes), "a child outside the node array"
        seen[i] += 1
        nd = nodes[i]
        stats["depth"] = max(stats["depth"], level)
        if nd["is_leaf"]:
            a, k = int(nd["idx"]), int(nd["n_prims"])
            assert k >= 1 and a == next_prim[0], ("the leaves do not tile [0, n) in order", i, a, next_prim[0])
            next_prim[0] = b = a + k
            assert np.array_equal(nd["bmin"], lo[a:b].min(axis=0)) and np.array_equal(nd["bmax"], hi[a:b].max(axis=0)), ("a leaf's box is not the union of its primitives' bounds", i)
            if k > 1:
                assert (cen[a:b].view(np.uint32) == cen[a].view(np.uint32)).all(), ("a leaf of several primitives whose centroids differ", i)
            stats["leaves"] += 1; stats["widest_leaf"] = max(stats["widest_leaf"], k)
            return i + 1, a, b
        stats["interior"] += 1
        end1, a, m = visit(i + 1, level + 1)          # pre-order: the first child follows its parent
        second = int(nd["idx"])
        assert second == end1 and second > i + 1, ("the second child does not follow the first child's subtree", i, second, end1)
        end2, m2, b = visit(second, level + 1)
        assert m2 == m
        c1, c2 = nodes[i + 1], nodes[second]
        assert np.array_equal(nd["bmin"], np.minimum(c1["bmin"], c2["bmin"])) and np.array_equal(nd["bmax"], np.maximum(c1["bmax"], c2["bmax"])), ("an interior box is not the join of its children's", i)
        cb_lo, cb_hi = cen[a:b].min(axis=0), cen[a:b].max(axis=0)
        assert not np.array_equal(cb_lo, cb_hi), ("an interior node over bit-equal centroids", i)
        ax = max_extent(cb_lo, cb_hi)
        assert int(nd["axis"]) == ax, ("split axis", i, int(nd["axis"]), ax)
        mid = F32(F32(cb_lo[ax] + cb_hi[ax]) / F32(2.0))                    # bvh.rs:99
        left, right = cen[a:m, ax], cen[m:b, ax]
        below = int((cen[a:b, ax] < mid).sum())
        if 0 < below < b - a:                         # :100-107: the middle split, as sets
            assert (left < mid).all() and (right >= mid).all(), ("the middle split's sides", i)
        else:                                         # :122-131: equal counts
            stats["fallbacks"] += 1
            assert m - a == (b - a) // 2 and left.max() <= right.min(), ("the equal-counts fallback's sides", i)
        return end2, a, b

    end, a, b = visit(0, 0)                           # (the reference's own stack holds 64 nodes: no tree here is deeper)
    assert end == len(nodes) and (seen == 1).all(), "a node is reached twice or never"
    assert (a, b) == (0, n)
    assert stats["depth"] == depth, ("reported depth", depth, "real", stats["depth"])
    return stats


def check_lights(builder, kind, prim, order):
    """Scene::new (scene/mod.rs:32-49): the explicit lights in the builder's order, then one area light per emitting primitive in strictly increasing BVH
    primitive index.  kind / prim: scene_get_lights (prim = the BVH index of an area light's primitive, < 0 otherwise) -> the emitters' builder indices
    in the order of Scene::lights"""
    n_explicit = len(builder.lights)
    emit = []
    for p in builder.prims:
        emit += [p[4] >= 0] * p[2] if p[0] == "trirange" else [p[3] >= 0]
    emitting = set(np.flatnonzero(emit).tolist())
    assert len(kind) == len(prim) == n_explicit + len(emitting)
    assert [int(k) for k in kind[:n_explicit]] == [int(l.type) for l in builder.lights] and (np.asarray(prim[:n_explicit]) < 0).all(), "the explicit lights come first, in the builder's order"
    area = np.asarray(prim[n_explicit:], np.int64)
    assert (area >= 0).all() and (np.diff(area) > 0).all(), "the area lights are not in strictly increasing BVH primitive index"
    got = [int(order[p]) for p in area]
    assert set(got) == emitting and len(got) == len(emitting), "not one area light per emitting primitive"
    return got


# ------------------------------------------------------------------ layer B
class Judgement:
    """[rays x primitives]: t (binary64), hit (binary64 says hit), doubt (binary32 may decide otherwise), bound (what t may differ by)"""

    def __init__(self, builder, geo, rays):
        o, d, t_max = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64), rays[:, 6].astype(np.float64)
        R, P = len(rays), len(geo)
        self.t, self.bound = np.full((R, P), np.nan), np.full((R, P), np.nan)
        self.hit, self.doubt = np.zeros((R, P), bool), np.zeros((R, P), bool)
        self.is_tri = np.array([g.kind == "tri" for g in geo])
        self.t_max = t_max
        with np.errstate(all="ignore"):
            for p, g in enumerate(geo):
                if g.kind == "tri":
                    h = g.hit_test(o, d, t_max, exact_origin=True)
                    t, hit, bound = h["t"], ~h["miss"], h["delta_t"]
                    doubt = h["fragile"] | h["nan_edges"]
                else:
                    r = g.intersect(o, d, t_max)
                    hit, t = r[0], r[6]
                    doubt, bound = IG.SceneRef.sphere_fragile(None, g, o, d, t_max, with_reach=True)
                # behind the origin or clearly beyond t_max: a miss in binary32 as well (SceneRef.intersect / occluded)
                doubt = doubt & ~(t <= 0.0) & ~(t > t_max * (1.0 + 1.0e-4))
                self.t[:, p], self.hit[:, p], self.doubt[:, p], self.bound[:, p] = t, hit, doubt, bound
            self.firm_hit, self.firm_miss = self.hit & ~self.doubt, ~self.hit & ~self.doubt
            tf = np.where(self.firm_hit, self.t, np.inf)
            self.prim = np.where(self.firm_hit.any(axis=1), np.argmin(tf, axis=1), -1)
            self.nearest = tf.min(axis=1)
            two = np.partition(tf, 1, axis=1)[:, :2] if P > 1 else np.stack([tf[:, 0], np.full(R, np.inf)], axis=1)
            tie = np.isfinite(two[:, 0]) & (two[:, 1] - two[:, 0] <= 1.0e-5 * np.abs(two[:, 0]))
            in_front = (self.doubt & ~(self.t > (self.nearest * (1.0 + 1.0e-4))[:, None])).any(axis=1)
        self.any_doubt = self.doubt.any(axis=1)
        self.pinned = ~in_front & ~tie
        for a in (self.t, self.bound, self.hit, self.doubt, self.firm_hit, self.firm_miss, self.prim, self.nearest, self.pinned, self.any_doubt):
            a.setflags(write=False)


def judge(builder, rays):
    import _interaction_common as IK
    return Judgement(builder, IK.geometry(builder), rays)


@functools.lru_cache(maxsize=3)
def judgement(name, family):
    """the judgement of one (scene, family) of _traversal_common, shared by the tests of a process that need it one after the other"""
    b, geo = C.description(name)
    return Judgement(b, geo, C.rays(name, family))


def builder_index(prim, order):
    """a library's BVH primitive indices (-1 = miss) -> the builder's"""
    prim, order = np.asarray(prim, np.int64), np.asarray(order, np.int64)
    return np.where(prim >= 0, order[np.maximum(prim, 0)], -1)


def check_closest(J, t, prim, what, bary=None):
    """a library's closest hits (prim: the builder's index, -1 = miss) on every row -> the largest |t - t64| / bound"""
    t, prim = np.asarray(t, np.float64), np.asarray(prim, np.int64)
    rows = np.arange(len(t))
    hit = prim >= 0
    with np.errstate(all="ignore"):
        bad = ~hit & J.firm_hit.any(axis=1)
        assert not bad.any(), (what, "a miss although a primitive is a firm hit", np.flatnonzero(bad)[:8])
        assert np.isinf(t[~hit]).all() and (t[~hit] > 0).all(), (what, "a miss whose t is not +inf")
        p = np.maximum(prim, 0)
        bad = hit & J.firm_miss[rows, p]
        assert not bad.any(), (what, "a hit on a primitive that is a firm miss", np.flatnonzero(bad)[:8])
        err, bound = np.abs(t - J.t[rows, p]), J.bound[rows, p]
        bad = hit & ~(err <= bound)
        assert not bad.any(), (what, "t further from the binary64 t than the pair's bound", np.flatnonzero(bad)[:8], err[bad][:8], bound[bad][:8])
        bad = hit & ~(t <= J.t_max)
        assert not bad.any(), (what, "t beyond t_max", np.flatnonzero(bad)[:8])
        nearer = J.firm_hit & (J.t + J.bound < t[:, None])
        bad = hit & nearer.any(axis=1)
        assert not bad.any(), (what, "a firm hit nearer than the reported t by more than its bound", np.flatnonzero(bad)[:8])
        bad = J.pinned & (prim != J.prim)
        assert not bad.any(), (what, "another primitive (or hit / miss) than brute force on a pinned row", np.flatnonzero(bad)[:8], prim[bad][:8], J.prim[bad][:8])
        if bary is not None:
            tri = hit & J.is_tri[p]
            s = np.asarray(bary, F32)[tri].astype(np.float64).sum(axis=1)
            assert (np.abs(s - 1.0) <= 4.0 * 2.0 ** -23).all(), (what, "barycentrics do not sum to 1 within 4 ulp", float(np.abs(s - 1.0).max()))
        ratio = np.where(hit & (bound > 0.0), err / bound, 0.0)
    return float(ratio.max()) if len(ratio) else 0.0


def check_occluded(J, occ, prim, what):
    """a library's any-hit answers on every row; prim: the same library's closest hits"""
    occ, hit = np.asarray(occ, bool), np.asarray(prim) >= 0
    bad = ~occ & J.firm_hit.any(axis=1)
    assert not bad.any(), (what, "not occluded although a primitive is a firm hit", np.flatnonzero(bad)[:8])
    bad = occ & J.firm_miss.all(axis=1)
    assert not bad.any(), (what, "occluded although every primitive is a firm miss", np.flatnonzero(bad)[:8])
    bad = ~J.any_doubt & (occ != hit)
    assert not bad.any(), (what, "occluded != (closest hit exists) where no primitive is doubtful", np.flatnonzero(bad)[:8])


def exact_zero_edges(geo, rays, faces):
    """per ray: whether an edge function of a face around its target is exactly 0 in the reference's arithmetic -- triangle.rs:186-223 in binary32, the
    binary64 products of :219-223 where one of them is 0.  sign_differs (:428-434) then goes by the zero's sign bit: the reference may miss every face
    around a vertex or an edge point that a ray passes through exactly (a named quirk)"""
    row = np.array([r for r, fs in enumerate(faces) for _ in fs])
    P = np.array([geo[f].p for fs in faces for f in fs]).astype(F32)              # [pairs, vertex, xyz]
    o, d = rays[row, 0:3].astype(F32), rays[row, 3:6].astype(F32)
    pt = P - o[:, None, :]
    kz = np.argmax(np.abs(d), axis=1)
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    i = np.arange(len(row))
    with np.errstate(all="ignore"):
        sx, sy = -d[i, kx] / d[i, kz], -d[i, ky] / d[i, kz]
        x = (pt[i, :, kx] + sx[:, None] * pt[i, :, kz]).astype(F32)
        y = (pt[i, :, ky] + sy[:, None] * pt[i, :, kz]).astype(F32)
        edges = lambda x, y: np.stack([x[:, 1] * y[:, 2] - y[:, 1] * x[:, 2], x[:, 2] * y[:, 0] - y[:, 2] * x[:, 0], x[:, 0] * y[:, 1] - y[:, 0] * x[:, 1]], axis=1)
        e = edges(x, y)
        again = (e == 0.0).any(axis=1)
        e[again] = edges(x[again].astype(np.float64), y[again].astype(np.float64)).astype(F32)
    out = np.zeros(len(faces), bool)
    np.logical_or.at(out, row, (e == 0.0).any(axis=1))
    return out


def check_seams(J, geo, rays, t, prim, occ, faces, what):
    """rays toward vertices and edge midpoints of a watertight mesh: every one hits and is occluded, at |t - 1| within the delta_t of the nearest
    face around the target, on one of those faces -- but for the rays through a target exactly (exact_zero_edges), which the generic rules judge
    -> (those rays, which of them leaked)"""
    t, prim, occ = np.asarray(t, np.float64), np.asarray(prim, np.int64), np.asarray(occ, bool)
    zero = exact_zero_edges(geo, rays, faces)
    bad = ~zero & ((prim < 0) | ~occ)
    assert not bad.any(), (what, "a ray through a seam", np.flatnonzero(bad)[:8])
    for r, fs in enumerate(faces):
        if zero[r]:
            continue
        assert prim[r] in fs, (what, "the face hit is not one around the target", r, int(prim[r]), fs)
        near = min(fs, key=lambda f: abs(J.t[r, f] - 1.0) if np.isfinite(J.t[r, f]) else np.inf)
        assert abs(t[r] - 1.0) <= J.bound[r, near], (what, "|t - 1| beyond the nearest adjacent face's delta_t", r, t[r], J.bound[r, near])
    return zero, zero & ((prim < 0) | ~occ)
