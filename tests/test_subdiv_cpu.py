"""Loop subdivision without a GPU (include/fountain_hip_subdiv.h): the host twin, which shares its per-element code with the kernels,
against the float64 restatement of tests/_subdiv_ref.py, and properties no reading of the rules enters: the counts' recurrences, the Euler
characteristic of every component, limit points inside the control points' box, planar meshes staying planar, affine covariance, the
octahedron's symmetry group, normals on the winding's side and of unit length, thread-count independence, and level l of level m's
topology being level l + m's.  The neighbour table is internal to the library: it is checked through the last property (the second run
rebuilds it from the child faces through the edge map, and the numbering of the next level's vertices follows from it) and through the
restatement, which rebuilds everything from the faces at every level."""
import numpy as np
import pytest

from fountain_amd import subdiv

import _subdiv_common as K
import _subdiv_ref as R

F32, F64 = np.float32, np.float64
_twin = {}


def twin(ftn, name, level):
    if (name, level) not in _twin:
        P, idx = K.mesh(name)
        _twin[(name, level)] = subdiv.loop_subdivide_cpu(ftn, P, idx, level)
    return _twin[(name, level)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name,level", K.CASES, ids=K.CASE_IDS)
def test_twin_matches_the_restatement(ftn, name, level):
    P, idx = K.mesh(name)
    got_P, got_N, got_idx = twin(ftn, name, level)
    want_P, want_N, want_idx = R.subdivide(P, idx, level, key=name)
    assert got_idx.dtype == np.uint32 and np.array_equal(got_idx.astype(np.int64), want_idx)
    ep, en = K.err(got_P, want_P, K.extent(P)), K.err(got_N, want_N, 1.0)
    print("%s level %d: P %.3g N %.3g" % (name, level, ep, en))
    assert ep <= 4.0 * K.MEASURED_P and en <= 4.0 * K.MEASURED_N


def test_levels_zero_keeps_the_faces(ftn):
    for name in K.SMALL:
        P, idx = K.mesh(name)
        assert np.array_equal(twin(ftn, name, 0)[2], idx)


@pytest.mark.parametrize("name", sorted(K.SMALL) + sorted(K.LARGE))
def test_counts_follow_the_recurrences(ftn, name):
    P, idx = K.mesh(name)
    top = K.LARGE[name][1] if name in K.LARGE else 4
    info = subdiv.info(ftn, idx, P.shape[0], top)
    assert info.levels == top
    chi = R.euler_characteristics(idx, P.shape[0])
    for l in (range(top + 1) if name in K.SMALL else (top,)):
        got_P, _, got_idx = twin(ftn, name, l)
        V, F, E = got_P.shape[0], got_idx.shape[0], R.edges(got_idx).shape[0]
        assert (info.n_vertices[l], info.n_faces[l], info.n_edges[l]) == (V, F, E)
        assert sorted(np.unique(got_idx)) == list(range(V))
        assert R.euler_characteristics(got_idx, V) == chi                                   # V - E + F of every component
        # boundary vertices: those on an edge that one face uses
        e = np.sort(np.concatenate([got_idx[:, [0, 1]], got_idx[:, [1, 2]], got_idx[:, [2, 0]]]).astype(np.int64), 1)
        u, c = np.unique(e, axis=0, return_counts=True)
        assert info.n_boundary[l] == np.unique(u[c == 1]).size and c.max() <= 2
    for l in range(top):
        assert info.n_faces[l + 1] == 4 * info.n_faces[l] and info.n_vertices[l + 1] == info.n_vertices[l] + info.n_edges[l]
        assert info.n_edges[l + 1] == 2 * info.n_edges[l] + 3 * info.n_faces[l]
    assert all(info.n_faces[l] == 0 and info.n_vertices[l] == 0 for l in range(top + 1, 11))


def test_counts_of_known_meshes(ftn):
    P, idx = K.mesh("octahedron")
    i = subdiv.info(ftn, idx, 6, 3)
    assert list(zip(i.n_vertices, i.n_faces))[:4] == [(6, 8), (18, 32), (66, 128), (258, 512)] and i.max_valence == 4
    P, idx = K.mesh("grid4")
    i = subdiv.info(ftn, idx, 16, 3)
    assert list(zip(i.n_vertices, i.n_faces))[:4] == [(16, 18), (49, 72), (169, 288), (625, 1152)]
    assert list(i.n_boundary)[:4] == [12, 24, 48, 96] and i.max_valence == 6
    assert subdiv.info(ftn, K.mesh("fan7")[1], 8, 0).max_valence == 7 and subdiv.info(ftn, K.mesh("tetrahedron")[1], 4, 0).max_valence == 3


@pytest.mark.parametrize("name,level", K.CASES, ids=K.CASE_IDS)
def test_limit_points_and_normals(ftn, name, level):
    """every weight is convex, so a limit point lies in the control points' box (to the rounding of the sums); the normal has length 1 to
    2 ulp and lies on the side of the incident faces' own winding"""
    P, idx = K.mesh(name)
    got_P, got_N, got_idx = twin(ftn, name, level)
    slack = 8 * 2.0 ** -24 * np.abs(P.astype(F64)).max()
    assert (got_P >= P.min(0) - slack).all() and (got_P <= P.max(0) + slack).all()
    assert np.abs(np.linalg.norm(got_N.astype(F64), axis=1) - 1.0).max() <= 2 * 2.0 ** -23
    fn = R.face_normal_sums(got_P, got_idx)
    cos = (fn * got_N).sum(1) / np.linalg.norm(fn, axis=1)
    print("%s level %d: worst cosine %.4f" % (name, level, cos.min()))
    assert cos.min() > 0.0
    if level >= 2:
        assert cos.min() > 0.99


def test_planar_meshes_stay_planar(ftn):
    rot = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]], F64)          # a rotation with exact entries
    for name, (P, idx) in (("triangle", K.triangle()), ("quad", _flat(K.quad())), ("grid", K.grid(5, bump=0.0)), ("fan", _flat(K.fan(7)))):
        Pr = (P.astype(F64) @ rot.T + [0.5, -2.0, 1.0]).astype(F32)
        p0, n = Pr[idx[0]].astype(F64), None
        n = np.cross(p0[1] - p0[0], p0[2] - p0[0])
        n /= np.linalg.norm(n)
        for level in (0, 1, 3):
            got_P, got_N, _ = subdiv.loop_subdivide_cpu(ftn, Pr, idx, level)
            off = np.abs((got_P.astype(F64) - p0[0]) @ n).max()
            assert off <= 32 * 2.0 ** -24 * np.abs(Pr).max(), (name, level, off)
            assert ((got_N.astype(F64) @ n) > 1.0 - 1e-4).all(), (name, level)


def _flat(m):
    P, idx = m
    P = P.copy()
    P[:, 2] = 0.0
    return P, idx


AFFINE_A = np.array([[1.5, 0.25, -0.5], [0.0, 0.75, 0.5], [0.25, -0.5, 2.0]], F64)
AFFINE_B = np.array([3.0, -1.0, 0.5], F64)


def test_affine(ftn):
    """subdivide(A P + b) = A subdivide(P) + b: 2e-15 in float64 (checked here with the restatement), the binary32 bound is measured"""
    worst = 0.0
    for name in ("fan7", "open_fan5", "tetrahedron", "icosahedron", "grid4"):
        P, idx = K.mesh(name)
        Q = (P.astype(F64) @ AFFINE_A.T + AFFINE_B).astype(F32)
        want = twin(ftn, name, 3)[0].astype(F64) @ AFFINE_A.T + AFFINE_B
        got_P, _, got_idx = subdiv.loop_subdivide_cpu(ftn, Q, idx, 3)
        assert np.array_equal(got_idx, twin(ftn, name, 3)[2])
        worst = max(worst, K.err(got_P, want, K.extent(Q)))
        if name == "fan7":
            ref = R.subdivide(P, idx, 2)[0] @ AFFINE_A.T + AFFINE_B
            assert K.err(R.subdivide(P.astype(F64) @ AFFINE_A.T + AFFINE_B, idx, 2)[0], ref, K.extent(Q)) <= 1e-13
    print("affine: %.3g" % worst)
    assert worst <= 4.0 * K.MEASURED_AFFINE


def test_octahedron_symmetry(ftn):
    """each of the 48 signed permutations of the axes maps the level-3 limit points and normals onto themselves"""
    import itertools
    got_P, got_N, _ = twin(ftn, "octahedron", 3)
    pts = np.concatenate([got_P, got_N], 1).astype(F64)
    key = lambda a: np.round(a * 1e4).astype(np.int64)
    have = set(map(tuple, key(pts)))
    assert len(have) == pts.shape[0]
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            m = pts[:, list(perm) + [3 + p for p in perm]] * np.array(signs + signs)
            assert set(map(tuple, key(m))) == have, (perm, signs)


def test_thread_count_changes_no_bit(ftn, monkeypatch):
    P, idx = K.mesh("grid25")
    level = K.LARGE["grid25"][1]
    monkeypatch.setenv("FTN_BVH_THREADS", "1")
    one = subdiv.loop_subdivide_cpu(ftn, P, idx, level)
    for threads in ("3", "16"):
        monkeypatch.setenv("FTN_BVH_THREADS", threads)
        got = subdiv.loop_subdivide_cpu(ftn, P, idx, level)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, one)), threads
    monkeypatch.delenv("FTN_BVH_THREADS")
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(twin(ftn, "grid25", level), one))


@pytest.mark.parametrize("name", ["quad", "fan7", "open_fan5", "tetrahedron", "grid4", "two_components"])
def test_level_l_of_level_m_is_level_l_plus_m(ftn, name):
    """the faces of level m, given as a control mesh, refine to the faces of level l + m: the second run rebuilds the neighbours and the
    start faces from the child faces, the first carried them through the closed forms"""
    P, idx = K.mesh(name)
    for m, l in ((1, 1), (1, 2), (2, 2), (3, 1)):
        mid_P, _, mid_idx = twin(ftn, name, m)
        again = subdiv.loop_subdivide_cpu(ftn, mid_P, mid_idx, l)[2]
        assert np.array_equal(again, twin(ftn, name, l + m)[2]), (m, l)


def test_inputs_untouched_and_repeatable(ftn):
    P, idx = K.mesh("icosahedron")
    P0, idx0 = P.copy(), idx.copy()
    a = subdiv.loop_subdivide_cpu(ftn, P, idx, 2)
    b = subdiv.loop_subdivide_cpu(ftn, P, idx, 2)
    assert np.array_equal(bits(P), bits(P0)) and np.array_equal(idx, idx0)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_python_interface(ftn, orc):
    import fountain_amd
    assert fountain_amd.loop_subdivide is subdiv.loop_subdivide and "loop_subdivide_cpu" in fountain_amd.__all__
    P, idx = K.mesh("octahedron")
    # over the oracle backend the product library's twin runs: the same bits
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(subdiv.loop_subdivide_cpu(orc, P, idx, 2), twin(ftn, "octahedron", 2)))
    with pytest.raises(fountain_amd.FountainError):
        subdiv.loop_subdivide(orc, P, idx, 1)
    with pytest.raises(ValueError):
        subdiv.loop_subdivide_cpu(ftn, P.ravel(), idx, 1)
