"""Which tables a scene keeps resident (Scene.info(): the fields of ftn_scene_memory), per build knob and per kind of scene.

The kernels fall back from one table to another (shading records -> prim_info and the vertex arrays, eight-box -> four-box -> two-box -> node
records, cell records -> the texel and function tables), so most parity tests still pass when a scene is created without a table it should hold,
or with one it should not.  These tests pin the tables themselves.  Sizes follow from the layouts of ftn_device.h: a node record is 32 bytes, a
shading record 128, a leaf-test record 48, a class one byte, a two-box record 64, a four-box record 128 and its quantised twin 64, an eight-box
record 128, an explicit leaf box 32, prim_info 32 per primitive, N / UV / T 12 / 8 / 12 per vertex.  Record counts come from the host builders'
own entry points (ftn_bvh_quads, ftn_bvh_octs) over the nodes the scene reports.

The knobs are read when the scene is created: they are set through `monkeypatch` around create_scene alone."""
import ctypes as C

import numpy as np
import pytest

from fountain_amd import SceneBuilder, _abi as A

pytestmark = pytest.mark.gpu

f32 = np.float32
KNOBS = ("FTN_TRACE4", "FTN_QUAD", "FTN_FAT", "FTN_QUAD64", "FTN_OCT", "FTN_SREC", "FTN_GEOM", "FTN_LEGACY_ARRAYS", "FTN_ENV_CELLS", "FTN_NO_COARSE_CDF")
K = 3                                                   # a K x K grid of quads: 18 triangles over 16 vertices, every leaf one triangle
N_TRI, N_VERT = 2 * K * K, (K + 1) * (K + 1)
DLIGHT, DIMAGE, TEXTURE, MTEX = 280, 208, 48, 32        # sizeof DLight, DImage (ftn_device.h), ftn_texture, ftn_material_textures (fountain_hip.h)


def grid(b, tangents=False):
    """a bumpy K x K grid with normals and uvs, away from every coordinate plane (no zero coordinate, no shared centroid)"""
    j, i = np.meshgrid(np.arange(K + 1), np.arange(K + 1), indexing="ij")
    P = np.stack([1.25 + i, 2.5 + 1.5 * j, 3.0 + 0.125 * ((i * 3 + j * 5) % 4)], -1).reshape(-1, 3).astype(f32)
    N = np.tile(np.array([0.0, 0.0, 1.0], f32), (N_VERT, 1))
    uv = np.stack([i / K, j / K], -1).reshape(-1, 2).astype(f32)
    idx = []
    for y in range(K):
        for x in range(K):
            v = y * (K + 1) + x
            idx += [(v, v + 1, v + K + 2), (v, v + K + 2, v + K + 1)]
    S = np.tile(np.array([1.0, 0.0, 0.0], f32), (N_VERT, 1)) if tangents else None
    b.shape("trianglemesh", P=P, N=N, uv=uv, indices=idx, S=S)


def create(b, monkeypatch, **knobs):
    with monkeypatch.context() as mp:
        for k in KNOBS:
            mp.delenv(k, raising=False)
        for k, v in knobs.items():
            mp.setenv(k, v)
        scene = b.create_scene()
    return scene, scene.info()


def mesh_scene(gpu, monkeypatch, sphere=False, tangents=False, **knobs):
    b = SceneBuilder(gpu)
    b.material("matte")
    grid(b, tangents)
    if sphere:
        b.attribute_begin(); b.translate((9.0, 9.0, 9.0)); b.shape("sphere", radius=0.5); b.attribute_end()
    return create(b, monkeypatch, **knobs)


def records(gpu, scene):
    """-> (interior nodes, leaves that are not one triangle, four-box records, eight-box records) of the scene's own BVH"""
    nodes = scene.nodes()[0]
    arr = np.ascontiguousarray(nodes)
    q = gpu.lib.ftn_bvh_quads
    q.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 3
    o = gpu.lib.ftn_bvh_octs
    o.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 5
    nq, no = C.c_uint32(), C.c_uint32()
    assert q(arr.ctypes.data_as(C.c_void_p), len(arr), None, C.byref(nq), None) == 0
    assert o(arr.ctypes.data_as(C.c_void_p), len(arr), None, C.byref(no), None, None, None) == 0
    leaf = nodes["is_leaf"] != 0
    return int((~leaf).sum()), int((leaf & (nodes["n_prims"] != 1)).sum()), nq.value, no.value


def check_common(i, n_prims):
    assert i["n_prims"] == n_prims
    assert i["nodes_bytes"] == 32 * i["n_nodes"] and i["prim_class_bytes"] == n_prims
    parts = ("nodes", "quad", "oct", "fat", "geom", "srec", "indexed_attributes", "prim_class", "lights", "textures", "other")
    assert i["total_bytes"] == sum(i[k + "_bytes"] for k in parts)


def test_triangle_only_defaults(gpu, monkeypatch):
    """leaf tests read the shading records; four-box records in both sizes and eight-box records; nothing the records replace"""
    sc, i = mesh_scene(gpu, monkeypatch)
    interior, fat_leaves, nq, no = records(gpu, sc)
    check_common(i, N_TRI)
    assert fat_leaves == 0 and nq > 0 and no > 0
    assert i["srec_bytes"] == 128 * N_TRI and i["geom_bytes"] == 0
    assert i["quad_bytes"] == (128 + 64) * nq and i["oct_bytes"] == 128 * no
    assert i["fat_bytes"] == 0 and i["indexed_attributes_bytes"] == 0
    assert i["lights_bytes"] == 0 and i["textures_bytes"] == 0


def test_a_sphere_keeps_the_dense_leaf_records(gpu, monkeypatch):
    sc, i = mesh_scene(gpu, monkeypatch, sphere=True)
    interior, fat_leaves, nq, no = records(gpu, sc)
    check_common(i, N_TRI + 1)
    assert i["geom_bytes"] == 48 * (N_TRI + 1) and i["srec_bytes"] == 128 * (N_TRI + 1)
    assert i["oct_bytes"] == 0 and i["quad_bytes"] == 128 * nq and nq > 0
    assert i["fat_bytes"] == 0 and i["indexed_attributes_bytes"] == 0


def test_without_shading_records(gpu, monkeypatch):
    sc, i = mesh_scene(gpu, monkeypatch, FTN_SREC="0")
    check_common(i, N_TRI)
    assert i["srec_bytes"] == 0 and i["geom_bytes"] == 48 * N_TRI
    assert i["indexed_attributes_bytes"] == 32 * N_TRI + (12 + 8) * N_VERT


def test_tangents_keep_the_indexed_attributes(gpu, monkeypatch):
    sc, i = mesh_scene(gpu, monkeypatch, tangents=True)
    check_common(i, N_TRI)
    assert i["srec_bytes"] == 128 * N_TRI and i["geom_bytes"] == 0
    assert i["indexed_attributes_bytes"] == 32 * N_TRI + (12 + 8 + 12) * N_VERT


def test_build_knobs_of_the_record_trees(gpu, monkeypatch):
    sc, base = mesh_scene(gpu, monkeypatch)
    interior, fat_leaves, nq, no = records(gpu, sc)
    sc, i = mesh_scene(gpu, monkeypatch, FTN_QUAD="0")
    check_common(i, N_TRI)
    assert i["quad_bytes"] == 0 and i["oct_bytes"] == 0 and i["fat_bytes"] == 64 * interior and interior > 0
    sc, i = mesh_scene(gpu, monkeypatch, FTN_OCT="0")
    check_common(i, N_TRI)
    assert i["oct_bytes"] == 0 and i["quad_bytes"] == base["quad_bytes"] and i["fat_bytes"] == 0
    sc, i = mesh_scene(gpu, monkeypatch, FTN_QUAD64="0")
    check_common(i, N_TRI)
    assert i["quad_bytes"] == 128 * nq and i["oct_bytes"] == base["oct_bytes"]
    for knobs in (dict(FTN_FAT="1"), dict(FTN_TRACE4="0")):
        sc, i = mesh_scene(gpu, monkeypatch, **knobs)
        check_common(i, N_TRI)
        assert i["fat_bytes"] == 64 * interior and i["quad_bytes"] == base["quad_bytes"] and i["oct_bytes"] == base["oct_bytes"]
    sc, i = mesh_scene(gpu, monkeypatch, FTN_GEOM="1")
    check_common(i, N_TRI)
    assert i["geom_bytes"] == 48 * N_TRI and i["srec_bytes"] == 128 * N_TRI and i["indexed_attributes_bytes"] == 0
    sc, i = mesh_scene(gpu, monkeypatch, FTN_LEGACY_ARRAYS="1")
    check_common(i, N_TRI)
    assert i["srec_bytes"] == 128 * N_TRI and i["indexed_attributes_bytes"] == 32 * N_TRI + (12 + 8) * N_VERT


def env_tables(w, h, cells, coarse):
    """bytes of an infinite light's tables for a w x h map.  compute_distribution swaps the names: the distribution has nv = w rows of
    nu = h entries.  texels (float4), function, conditional CDFs, conditional integrals and their copy as the marginal function, marginal
    CDF; cell records; every 32nd entry of each CDF"""
    nu, nv = h, w
    n = 16 * w * h + 4 * (nu * nv + nv * (nu + 1) + nv + nv + (nv + 1))
    if cells:
        n += 128 * w * h
    if coarse:
        n += 4 * (nv * ((nu + 31) // 32 + 1) + (nv + 31) // 32 + 1)
    return n


def env_scene(gpu, monkeypatch, w, h, **knobs):
    b = SceneBuilder(gpu)
    rng = np.random.default_rng(w * 100 + h)
    b.light_source("infinite", texels=rng.uniform(0.05, 1.0, (h, w, 3)).astype(f32))
    b.material("matte")
    b.shape("sphere", radius=1.0)
    return create(b, monkeypatch, **knobs)[1]


def test_environment_tables(gpu, monkeypatch):
    """a square map has cell records (128 bytes per texel), any other has not; FTN_ENV_CELLS=0 and FTN_NO_COARSE_CDF drop their tables alone"""
    one = DLIGHT + 4
    square, wide = env_scene(gpu, monkeypatch, 40, 40), env_scene(gpu, monkeypatch, 40, 24)
    assert square["lights_bytes"] == one + env_tables(40, 40, True, True)
    assert wide["lights_bytes"] == one + env_tables(40, 24, False, True)
    assert env_scene(gpu, monkeypatch, 40, 40, FTN_ENV_CELLS="0")["lights_bytes"] == one + env_tables(40, 40, False, True) == square["lights_bytes"] - 128 * 40 * 40
    assert env_scene(gpu, monkeypatch, 40, 40, FTN_ENV_CELLS="1")["lights_bytes"] == square["lights_bytes"]
    for value in ("1", "0"):                           # presence alone counts
        assert env_scene(gpu, monkeypatch, 40, 40, FTN_NO_COARSE_CDF=value)["lights_bytes"] == one + env_tables(40, 40, True, False)


def test_textures_and_pyramids(gpu, monkeypatch):
    b = SceneBuilder(gpu)
    rng = np.random.default_rng(7)
    b.texture("img", "spectrum", "imagemap", texels=rng.uniform(0.0, 1.0, (3, 5, 3)).astype(f32))       # 5 x 3: levels 5x3, 2x1, 1x1
    b.texture("big", "spectrum", "imagemap", texels=rng.uniform(0.0, 1.0, (8, 8, 3)).astype(f32), wrap="clamp")   # 8x8, 4x4, 2x2, 1x1
    b.texture("chk", "spectrum", "checkerboard", tex1="img", tex2=(0.8, 0.7, 0.6))
    b.material("matte", Kd="chk")
    grid(b)
    b.material("plastic", Ks="big")
    b.shape("sphere", radius=0.5)
    b.material("matte")
    b.shape("sphere", radius=0.25)
    i = create(b, monkeypatch)[1]
    n_textures, n_materials, n_images = len(b.textures), len(b.materials), len(b.images)
    assert n_images == 2 and n_textures >= 3 and n_materials >= 3
    texels = (15 + 2 + 1) + (64 + 16 + 4 + 1)
    assert i["textures_bytes"] == TEXTURE * n_textures + MTEX * n_materials + DIMAGE * n_images + 16 * texels
    check_common(i, N_TRI + 2)
    sc, plain = mesh_scene(gpu, monkeypatch)
    assert plain["textures_bytes"] == 0
