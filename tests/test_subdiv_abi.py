"""The Loop subdivision extension of the C ABI (include/fountain_hip_subdiv.h) without a GPU: the header, the ctypes mirror and the
library's exports agree; the layout and the version; every refusal in the header's order for the info, GPU and twin entries (each stage
is tried with every later stage violated as well, and the message must be its own and name the smallest offending index); then
FTN_ERR_NO_DEVICE where there is no GPU; `Shape "loopsubdiv"` of the PBRT reader against the SceneBuilder calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fountain_amd import FountainError, PbrtScene, PerspectiveCamera, SceneBuilder, subdiv
from fountain_amd import _abi as A

import _subdiv_common as K
from test_pbrt_loader import assert_same_desc, same_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fountain_hip_subdiv.h")
F32 = np.float32
INV, NODEV = A.FTN_ERR_INVALID_ARGUMENT, A.FTN_ERR_NO_DEVICE


@pytest.fixture(scope="module")
def lib(ftn):
    return subdiv._lib(ftn)[1]


def header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ftn_[a-z0-9_]+)\s*\(", src)))


def last(ftn):
    return ftn.fn("last_error")().decode()


def test_header_mirror_and_exports_agree(ftn):
    assert header_functions() == sorted(A.SUBDIV_FUNCTIONS) == sorted(A.SUBDIV_PROTOTYPES)
    for other in (A.DECLARED_FUNCTIONS, A.GBUFFER_FUNCTIONS, A.DENOISE_FUNCTIONS, A.DENOISE_GUIDED_FUNCTIONS, A.MOMENTS_FUNCTIONS, A.ADAPTIVE_FUNCTIONS,
                  A.TEMPORAL_FUNCTIONS, A.FILTER_FUNCTIONS, A.DISPLAY_FUNCTIONS, A.BLOOM_FUNCTIONS):
        assert not set(A.SUBDIV_FUNCTIONS) & set(other)
    for name in A.SUBDIV_FUNCTIONS:
        assert hasattr(ftn.lib, name), "libfountain_hip.so does not export %s" % name
    assert "subdiv" not in open(os.path.join(ROOT, "include", "fountain_hip.h")).read()


def test_layout_versions_and_constants(ftn, lib):
    assert C.sizeof(A.ftn_subdiv_info) == 184 == A.SIZES["ftn_subdiv_info"]
    assert {name: getattr(A.ftn_subdiv_info, name).offset for name, _ in A.ftn_subdiv_info._fields_} == {
        "levels": 0, "max_valence": 4, "n_vertices": 8, "n_faces": 52, "n_edges": 96, "n_boundary": 140}
    header = open(HEADER).read()
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1))
    assert define("FTN_SUBDIV_ABI_VERSION") == A.FTN_SUBDIV_ABI_VERSION == 1 == lib.ftn_subdiv_abi_version()
    assert define("FTN_SUBDIV_MAX_LEVELS") == A.FTN_SUBDIV_MAX_LEVELS == 10 and A.FTN_SUBDIV_MAX_FACES == 1 << 26
    # the main ABI and the other extensions are unchanged
    assert ftn.lib.ftn_abi_version() == A.FTN_ABI_VERSION == 3
    assert ftn.lib.ftn_bloom_abi_version() == 1 and ftn.lib.ftn_display_abi_version() == 1 and ftn.lib.ftn_filter_abi_version() == 1


# ------------------------------------------------------------------ refusals, in the header's order
# (stage, the words its message must hold)
STAGES = [("null", "null argument"), ("counts", "must be positive"), ("levels", "levels must be 0..10"), ("limit", "2^26"),
          ("range", "out of range in face 9"), ("repeated", "repeated vertex in face 10"), ("third", "more than two faces, the third is face 11"),
          ("winding", "inconsistent winding"), ("unused", "no face uses vertex"), ("pinched", "pinched at vertex")]


class Call:
    """an octahedron and, for every topology stage that is on, the faces that violate it; host buffers large enough for any entry"""

    def __init__(self, on):
        is_on = lambda s: s in on
        faces = [list(t) for t in K.octahedron()[1]]
        nv = 6
        faces.append([6, 7, 8])                                                    # face 8 is in order; faces 9, 10 and 11 follow
        faces.append([0, 2, 4000] if is_on("range") else [9, 10, 11])
        faces.append([12, 12, 13] if is_on("repeated") else [12, 14, 13])
        faces.append([0, 2, 15] if is_on("third") else [15, 16, 17])              # the third face on the edge 0 - 2
        nv = 18
        if is_on("winding"):
            faces += [[nv, nv + 1, nv + 2], [nv, nv + 1, nv + 3]]
            self.winding_face = len(faces) - 1
            nv += 4
        if is_on("pinched"):
            faces += [[nv, nv + 1, nv + 2], [nv, nv + 3, nv + 4]]
            self.pinched_vertex = nv
            nv += 5
        if is_on("unused"):
            self.unused_vertex = nv
            nv += 1
        used = {v for t in faces for v in t if v < 4000}
        assert is_on("unused") or is_on("range") or used == set(range(nv))
        self.idx = np.array(faces, np.uint32)
        self.levels = 11 if is_on("levels") else (10 if is_on("limit") else 1)
        if is_on("limit"):                                                         # 65 faces: 65 * 4^10 > 2^26
            extra = [[nv + 3 * i, nv + 3 * i + 1, nv + 3 * i + 2] for i in range(65 - len(faces))]
            self.idx = np.array(faces + extra, np.uint32)
            nv += 3 * len(extra)
        self.nv = 0 if is_on("counts") else nv
        self.P = np.arange(3 * nv, dtype=F32).reshape(-1, 3)
        self.out = np.zeros(4096, F32)
        self.null = is_on("null")

    def args(self, entry):
        i = None if self.null else self.idx.ctypes.data
        o = self.out.ctypes.data
        if entry == "loop_subdivide_info":
            return (i, self.nv, self.idx.shape[0], self.levels, o)
        base = (self.P.ctypes.data, self.nv, i, self.idx.shape[0], self.levels, o, o, o)
        return base + ((-1,) if entry == "loop_subdivide" else ())


ENTRIES = ["loop_subdivide_info", "loop_subdivide", "loop_subdivide_cpu"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_in_order(ftn, lib, entry):
    fn = getattr(lib, "ftn_" + entry)
    names = [s[0] for s in STAGES]
    for k, (first, words) in enumerate(STAGES):
        call = Call(set(names[k:]))
        assert fn(*call.args(entry)) == INV, (entry, first)
        assert words in last(ftn), (entry, first, last(ftn))
        if first == "winding":
            assert last(ftn).endswith("face %d" % call.winding_face)
        if first == "unused":
            assert last(ftn).endswith("vertex %d" % call.unused_vertex)
        if first == "pinched":
            assert last(ftn).endswith("vertex %d" % call.pinched_vertex)
        assert not call.out.any()
    call = Call(set())                                                             # nothing violated: the mesh itself is in order
    info = A.ftn_subdiv_info()
    assert lib.ftn_loop_subdivide_info(call.idx.ctypes.data, call.nv, call.idx.shape[0], 1, C.byref(info)) == 0 and info.n_faces[1] == 4 * 12


def test_further_refusals(ftn, lib):
    P, idx = K.octahedron()
    o = np.zeros(4096, F32)
    cpu = lambda P=P.ctypes.data, nv=6, idx=idx.ctypes.data, nf=8, levels=1, a=o.ctypes.data, b=o.ctypes.data, c=o.ctypes.data: \
        lib.ftn_loop_subdivide_cpu(P, nv, idx, nf, levels, a, b, c)
    assert cpu() == 0
    for kw in (dict(P=None), dict(idx=None), dict(a=None), dict(b=None), dict(c=None)):
        assert cpu(**kw) == INV and "null" in last(ftn), kw
    assert lib.ftn_loop_subdivide_info(idx.ctypes.data, 6, 8, 1, None) == INV and "null" in last(ftn)
    for kw in (dict(nv=0), dict(nv=-3), dict(nf=0), dict(nf=-1), dict(levels=-1), dict(levels=11)):
        assert cpu(**kw) == INV, kw
    assert cpu(levels=0) == 0
    # a Moebius strip of five triangles: every edge has at most two faces, no orientation is consistent
    strip = np.array([[0, 1, 2], [2, 1, 3], [2, 3, 4], [4, 3, 0], [4, 0, 1]], np.uint32)
    info = A.ftn_subdiv_info()
    assert lib.ftn_loop_subdivide_info(strip.ctypes.data, 5, 5, 1, C.byref(info)) == INV and "inconsistent winding" in last(ftn)
    # one flipped face of the octahedron; the later face of the pair is named
    flipped = idx.copy()
    flipped[3] = flipped[3][::-1]
    assert lib.ftn_loop_subdivide_info(flipped.ctypes.data, 6, 8, 1, C.byref(info)) == INV and "inconsistent winding" in last(ftn)
    # the smallest face is named when several are out of range
    bad = idx.copy()
    bad[5, 1] = 6
    bad[2, 0] = 77
    assert lib.ftn_loop_subdivide_info(bad.ctypes.data, 6, 8, 1, C.byref(info)) == INV and last(ftn).endswith("face 2")
    # a degenerate control mesh: every normal has zero length; the smallest vertex is named
    flat = np.zeros((6, 3), F32)
    assert cpu(P=flat.ctypes.data) == INV and "zero or non-finite" in last(ftn) and last(ftn).endswith("vertex 0")
    nan = P.copy()
    nan[4, 1] = np.nan
    assert cpu(P=nan.ctypes.data) == INV and "zero or non-finite" in last(ftn)
    with pytest.raises(FountainError):
        subdiv.loop_subdivide_cpu(ftn, flat, idx, 1)


def test_the_gpu_entry_reports_no_device(ftn, lib):
    """No CPU fallback: valid arguments and no device -> FTN_ERR_NO_DEVICE, after every refusal"""
    if ftn.fn("device_count")() > 0:
        pytest.skip("a GPU is present")
    P, idx = K.octahedron()
    o = np.zeros(4096, F32)
    for levels in (0, 2):
        assert lib.ftn_loop_subdivide(P.ctypes.data, 6, idx.ctypes.data, 8, levels, o.ctypes.data, o.ctypes.data, o.ctypes.data, -1) == NODEV
    assert "no CPU fallback" in last(ftn) and not o.any()
    with pytest.raises(FountainError) as e:
        subdiv.loop_subdivide(ftn, P, idx, 1)
    assert e.value.code == NODEV


# ------------------------------------------------------------------ the PBRT reader
SCENE = """
Film "image" "integer xresolution" [ 32 ] "integer yresolution" [ 32 ]
Sampler "random" "integer pixelsamples" 4
LookAt 3 -4 2.5  0 0 0  0 0 1
Camera "perspective" "float fov" 35
WorldBegin
LightSource "infinite" "rgb L" [0.9 1.0 1.2]
AttributeBegin
  Material "matte" "rgb Kd" [0.6 0.5 0.4]
  Rotate 20 0 0 1
  Scale 1.25 1 1
  Shape "loopsubdiv" %s "integer indices" [0 2 4  2 1 4  1 3 4  3 0 4  2 0 5  1 2 5  3 1 5  0 3 5]
        "point P" [1 0 0  -1 0 0  0 1 0  0 -1 0  0 0 1  0 0 -1]
AttributeEnd
AttributeBegin
  Material "plastic"
  Translate 0 0 -1.5
  Shape "loopsubdiv" "integer nlevels" 1 "integer indices" [0 1 2 0 2 3] "point P" [-3 -3 0  3 -3 0.5  3 3 0  -3 3 0.5]
AttributeEnd
WorldEnd
"""


def _built(be, levels):
    b = SceneBuilder(be)
    b.light_source("infinite", L=(0.9, 1.0, 1.2))
    P, idx = K.octahedron()
    b.attribute_begin(); b.material("matte", Kd=(0.6, 0.5, 0.4)); b.rotate(20, (0, 0, 1)); b.scale(1.25, 1, 1)
    b.shape("loopsubdiv", P=P, indices=idx, **levels)
    b.attribute_end()
    b.attribute_begin(); b.material("plastic"); b.translate((0, 0, -1.5))
    b.shape("loopsubdiv", nlevels=1, indices=[0, 1, 2, 0, 2, 3], P=[(-3, -3, 0), (3, -3, 0.5), (3, 3, 0), (-3, 3, 0.5)])
    b.attribute_end()
    return b, PerspectiveCamera.look_at(be, (3, -4, 2.5), (0, 0, 0), (0, 0, 1), (32, 32), fov=35.0)


@pytest.mark.parametrize("text,kw,faces", [('"integer levels" 2', dict(levels=2), 128), ('"integer nlevels" 1', dict(nlevels=1), 32), ("", dict(), 512),
                                           ('"integer levels" 0 "integer nlevels" 2', dict(levels=0), 8)])
def test_loopsubdiv_is_parsed_like_the_builder(ftn, tmp_path, text, kw, faces):
    (tmp_path / "s.pbrt").write_text(SCENE % text)
    ps = PbrtScene(str(tmp_path / "s.pbrt"), ftn)
    b, cam = _built(ftn, kw)
    d, keep = b.build_desc()
    assert_same_desc(ps.desc, d)
    assert same_struct(ps.camera.desc, cam.desc)
    assert ps.desc.n_triangles == faces + 8 and ps.desc.meshes[0].has_normals == 1 and ps.desc.meshes[1].has_normals == 1


def test_loopsubdiv_statement_refusals(ftn, tmp_path):
    def load(scene):
        (tmp_path / "bad.pbrt").write_text(scene)
        with pytest.raises(FountainError) as e:
            PbrtScene(str(tmp_path / "bad.pbrt"), ftn)
        return str(e.value)
    base = SCENE % ""
    assert "needs indices and P" in load(base.replace('"point P" [1 0 0  -1 0 0  0 1 0  0 -1 0  0 0 1  0 0 -1]', ""))
    assert "needs indices and P" in load(base.replace('"integer indices" [0 2 4  2 1 4  1 3 4  3 0 4  2 0 5  1 2 5  3 1 5  0 3 5]', ""))
    assert "levels must be 0..10" in load(SCENE % '"integer levels" 11')
    assert "inconsistent winding" in load(base.replace("[0 2 4  2 1 4", "[0 2 4  1 2 4"))
    assert "out of range in face 1" in load(base.replace("2 1 4  1 3 4", "2 9 4  1 3 4"))
    assert "not a multiple of 3" in load(base.replace("0 3 5]", "0 3 5 1]"))
    with pytest.raises(ValueError):
        SceneBuilder(ftn).shape("loopsubdiv", indices=[0, 1, 2])
    with pytest.raises(FountainError):
        SceneBuilder(ftn).shape("loopsubdiv", indices=[0, 1, 1], P=[(0, 0, 0), (1, 0, 0), (0, 1, 0)])
