"""Control meshes for the Loop subdivision tests (include/fountain_hip_subdiv.h), each there for the rule it reaches, the error measure and
the bounds measured with the host twin."""
import numpy as np

F32, F64 = np.float32, np.float64


def _mesh(P, idx):
    return np.ascontiguousarray(P, F32).reshape(-1, 3), np.ascontiguousarray(idx, np.uint32).reshape(-1, 3)


def triangle():
    """all boundary, valence 2"""
    return _mesh([[0, 0, 0], [1, 0, 0.25], [0.25, 1, 0.5]], [[0, 1, 2]])


def quad():
    """two triangles: boundary valence 3 at the shared edge's ends"""
    return _mesh([[0, 0, 0], [1, 0, 0.125], [1, 1, 0.5], [0, 1, 0.25]], [[0, 1, 2], [0, 2, 3]])


def fan(n, hub_z=0.5, closed=True, wobble=0.0625):
    """a hub and n rim vertices; closed: the hub is interior with valence n; open: n - 1 faces, the hub is on the boundary with valence n"""
    a = 2.0 * np.pi * np.arange(n) / n
    rim = np.stack([np.cos(a), np.sin(a), wobble * np.cos(3.0 * a)], 1)
    P = np.concatenate([[[0.0, 0.0, hub_z]], rim])
    idx = [[0, 1 + i, 1 + (i + 1) % n] for i in range(n if closed else n - 1)]
    return _mesh(P, idx)


def tetrahedron():
    """valence 3: the beta special case"""
    return _mesh([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def octahedron(scale=1.0):
    """valence 4"""
    P = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F64) * scale
    return _mesh(P, [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])


def icosahedron():
    """valence 5"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    P = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    idx = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
           [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    return _mesh(P, idx)


def grid(n, bump=0.25):
    """n x n vertices, 2 (n - 1)^2 faces: a regular interior (valence 6), boundary valences 2, 3 and 4; z = bump * a smooth bump"""
    y, x = np.mgrid[0:n, 0:n].astype(F64)
    z = bump * np.sin(1.3 * x + 0.2) * np.cos(0.9 * y - 0.4)
    P = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
    idx = []
    for j in range(n - 1):
        for i in range(n - 1):
            a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i + 1, (j + 1) * n + i
            idx += [[a, b, c], [a, c, d]]
    return _mesh(P, idx)


def two_components():
    """a tetrahedron and a quad that share nothing"""
    P0, i0 = tetrahedron()
    P1, i1 = quad()
    return _mesh(np.concatenate([P0, P1 + F32([4, 0, 0])]), np.concatenate([i0, i1 + np.uint32(P0.shape[0])]))


# name -> (mesh, levels); the small meshes at every level 0..4, the large grid (73 728 faces and 221 184 slots at level 3: several
# workgroups, several host threads, the scan over more than one workgroup's sum) at level 3 alone
SMALL = {
    "triangle": triangle, "quad": quad, "fan7": lambda: fan(7), "fan12_raised": lambda: fan(12, hub_z=1.5),
    "open_fan5": lambda: fan(5, closed=False), "open_fan7": lambda: fan(7, closed=False),          # the hub: boundary valence 5 and 7
    "tetrahedron": tetrahedron, "octahedron": octahedron, "icosahedron": icosahedron, "grid4": lambda: grid(4),
    "two_components": two_components, "octahedron_1e4": lambda: octahedron(1e4),
}
SMALL_LEVELS = (0, 1, 2, 3, 4)
LARGE = {"grid25": (lambda: grid(25), 3)}
CASES = [(name, l) for name in SMALL for l in SMALL_LEVELS] + [(name, l) for name, (_, l) in LARGE.items()]
CASE_IDS = ["%s-L%d" % c for c in CASES]


def mesh(name):
    return SMALL[name]() if name in SMALL else LARGE[name][0]()


def extent(P):
    P = np.asarray(P, F64)
    return float(np.linalg.norm(P.max(0) - P.min(0)))


def err(got, want, ext):
    """max |got - want| / max(|want|, 1e-3 ext), per component"""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-3 * ext))) if want.size else 0.0


# Measured with the host twin (ftn_loop_subdivide_cpu) against tests/_subdiv_ref.py on the CPU, the maximum over CASES; the tests allow
# 4 x these (DESIGN.md section 3.1's convention).  Never taken from a device run: the device is compared with the twin bit for bit.
MEASURED_P = 4.04e-6
MEASURED_N = 5.63e-3
# the same for subdivide(A P + b) against A subdivide(P) + b (positions; the meshes and the map of test_subdiv_cpu.test_affine)
MEASURED_AFFINE = 1.5e-5
