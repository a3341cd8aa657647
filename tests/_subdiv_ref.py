"""A float64 restatement of include/fountain_hip_subdiv.h that keeps no pointers: no start faces, no neighbour table, no walk.  Every
level rebuilds what it needs from the faces alone -- a map from an edge's unordered vertex pair to the faces' opposite vertices, and per
vertex the map "next -> previous" of the faces around it, from which a ring is chained.  Only the numbering of new vertices (the order of
first discovery in a serial loop over the faces) and the layout of a face's children are shared with the library, because the indices
must be identical.  An interior ring starts wherever this code happens to start it: in exact arithmetic neither a position nor
cross(T, S) depends on that."""
import math

import numpy as np

F64 = np.float64


def beta(n):
    return 3.0 / 16.0 if n == 3 else 3.0 / (8.0 * n)


def gamma(n):
    return 1.0 / (n + 3.0 / (8.0 * beta(n)))


def rings(idx, nv):
    """per vertex (ring, is_boundary) in the header's ring order: interior rings run against the faces' winding (r_{j+1} is the `next`
    of the face whose `previous` is r_j), boundary rings with it, from the vertex no face has as a `previous`"""
    nxt2prev = [dict() for _ in range(nv)]
    for a, b, c in idx:
        nxt2prev[a][b] = c; nxt2prev[b][c] = a; nxt2prev[c][a] = b
    out = []
    for v in range(nv):
        m = nxt2prev[v]
        prevs = set(m.values())
        starts = [a for a in m if a not in prevs]
        if starts:                                            # boundary
            assert len(starts) == 1
            ring = [starts[0]]
            while ring[-1] in m:
                ring.append(m[ring[-1]])
            out.append((ring, True))
        else:
            inv = {p: n for n, p in m.items()}
            first = next(iter(m))
            ring = [first]
            while inv[ring[-1]] != first:
                ring.append(inv[ring[-1]])
            out.append((ring, False))
        assert len(out[-1][0]) == len(m) + (1 if starts else 0)
    return out


def vertex_rule(P, v, ring, boundary, limit):
    if boundary:
        w = 0.2 if limit else 0.125
        return (1.0 - 2.0 * w) * P[v] + w * P[ring[0]] + w * P[ring[-1]]
    n = len(ring)
    w = gamma(n) if limit else beta(n)
    return (1.0 - n * w) * P[v] + w * P[ring].sum(0)


def one_level(P, idx):
    nv = P.shape[0]
    opposite = {}
    for a, b, c in idx:
        for u, w, o in ((a, b, c), (b, c, a), (c, a, b)):
            opposite.setdefault((min(u, w), max(u, w)), []).append(o)
    R = rings(idx, nv)
    new_P = [vertex_rule(P, v, R[v][0], R[v][1], False) for v in range(nv)]
    edge_vertex = {}
    new_idx = []
    for tri in idx:
        e = []
        for k in range(3):
            u, w = tri[k], tri[(k + 1) % 3]
            key = (min(u, w), max(u, w))
            if key not in edge_vertex:
                edge_vertex[key] = len(new_P)
                o = opposite[key]
                new_P.append(0.5 * P[u] + 0.5 * P[w] if len(o) == 1 else 0.375 * P[u] + 0.375 * P[w] + 0.125 * P[o[0]] + 0.125 * P[o[1]])
            e.append(edge_vertex[key])
        for j in range(3):
            child = [0, 0, 0]
            child[j], child[(j + 1) % 3], child[(j + 2) % 3] = tri[j], e[j], e[(j + 2) % 3]
            new_idx.append(child)
        new_idx.append(e)
    return np.array(new_P, F64), new_idx


def limit_surface(P, idx):
    nv = P.shape[0]
    R = rings(idx, nv)
    L = np.array([vertex_rule(P, v, R[v][0], R[v][1], True) for v in range(nv)], F64)
    N = np.zeros((nv, 3), F64)
    for v in range(nv):
        ring, boundary = R[v]
        n = len(ring)
        r = L[ring]
        if not boundary:
            a = 2.0 * math.pi * np.arange(n) / n
            S, T = (np.cos(a)[:, None] * r).sum(0), (np.sin(a)[:, None] * r).sum(0)
        else:
            S = r[-1] - r[0]
            if n == 2:
                T = r[0] + r[1] - 2.0 * L[v]
            elif n == 3:
                T = r[1] - L[v]
            elif n == 4:
                T = -r[0] + 2.0 * r[1] + 2.0 * r[2] - r[3] - 2.0 * L[v]
            else:
                th = math.pi / (n - 1)
                T = math.sin(th) * (r[0] + r[-1])
                for k in range(1, n - 1):
                    T = T + (2.0 * math.cos(th) - 2.0) * math.sin(k * th) * r[k]
                T = -T
        c = np.cross(T, S)
        N[v] = c / np.linalg.norm(c)
    return L, N


_cache = {}


def subdivide(P, idx, levels, key=None):
    """(limit positions, normals, indices [F, 3] int64) of the control mesh refined `levels` times, all float64; `key` caches the result"""
    if key is not None and (key, levels) in _cache:
        return _cache[(key, levels)]
    P = np.asarray(P, F64)
    idx = [[int(x) for x in t] for t in np.asarray(idx)]
    for _ in range(levels):
        P, idx = one_level(P, idx)
    L, N = limit_surface(P, idx)
    out = (L, N, np.array(idx, np.int64).reshape(-1, 3))
    if key is not None:
        _cache[(key, levels)] = out
    return out


def edges(idx):
    """the set of unordered vertex pairs"""
    idx = np.asarray(idx, np.int64)
    e = np.concatenate([idx[:, [0, 1]], idx[:, [1, 2]], idx[:, [2, 0]]])
    return np.unique(np.sort(e, 1), axis=0)


def components(idx, nv):
    """a component label per vertex (union-find over the edges)"""
    parent = list(range(nv))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in edges(idx):
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[rb] = ra
    return np.array([find(v) for v in range(nv)])


def euler_characteristics(idx, nv):
    """sorted V - E + F of every component"""
    idx = np.asarray(idx, np.int64)
    lab = components(idx, nv)
    e = edges(idx)
    return sorted(int((lab == c).sum() - (lab[e[:, 0]] == c).sum() + (lab[idx[:, 0]] == c).sum()) for c in np.unique(lab))


def face_normal_sums(P, idx):
    """per vertex the sum of cross(p1 - p0, p2 - p0) over its faces (area-weighted, on the winding's side)"""
    P, idx = np.asarray(P, F64), np.asarray(idx, np.int64)
    c = np.cross(P[idx[:, 1]] - P[idx[:, 0]], P[idx[:, 2]] - P[idx[:, 0]])
    out = np.zeros_like(P)
    for k in range(3):
        np.add.at(out, idx[:, k], c)
    return out
