"""Valid files do not change by a bit: the SHA-256 of every array of ftn_pbrt_scene, of the camera and of the film, for the scene texts
test_pbrt_loader.py and test_output_stage.py write (test_textures.py writes none), against tests/golden/reader_descriptors.json --
this project's own results, recorded before the readers learnt to refuse corrupt files (`python tests/test_reader_descriptors.py
--record` rewrites the file from the library as built).  Host only."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "reader_descriptors.json")


def _inputs(dirpath, ftn):
    """Every file the scene texts name, written once into dirpath."""
    from fountain_amd import scenes, write_exr
    from test_pbrt_loader import INC, _write_ply
    P, N, F = scenes.rounded_cube_mesh()
    _write_ply(os.path.join(dirpath, "cube.ply"), P, N, None, F, True)
    with open(os.path.join(dirpath, "inc.pbrt"), "w") as f:
        f.write(INC)
    write_exr(os.path.join(dirpath, "t.exr"), np.random.default_rng(4).random((6, 10, 3)).astype(np.float32), ftn)
    write_exr(os.path.join(dirpath, "sky.exr"), np.random.default_rng(2).random((8, 8, 3)).astype(np.float32), ftn)


def scene_texts():
    import test_output_stage as O
    import test_pbrt_loader as L
    gold = lambda n: open(os.path.join(L.GOLD, n)).read()
    return {
        "furnace_empty": gold("furnace_empty.pbrt"),
        "cornell": gold("cornell.pbrt"),
        "every_statement": L.FEATURES,
        "plastic_ks": 'Camera "perspective"\nWorldBegin\nMaterial "plastic" "rgb Ks" [1 1 1]\nShape "sphere"\nWorldEnd\n',
        "textured": L.TEXTURED,
        "plymesh": L.PLYMESH_SCENE,
        "tangents": L.TANGENT_SCENE,
        "infinite_mapname": O.MAPNAME_SCENE,
    }


def _sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


def descriptor_hashes(ps):
    from test_pbrt_loader import desc_arrays
    out = {}
    for k, v in desc_arrays(ps.desc).items():
        if k in ("images", "envmaps"):
            out[k] = [_sha(np.asarray(x[:-1], np.uint32), x[-1]) for x in v]
        else:
            out[k] = "absent" if v is None else _sha(np.asarray(v.shape, np.uint32), v)
    out["camera"] = _sha(C.string_at(C.byref(ps.camera.desc), C.sizeof(ps.camera.desc)))
    out["film"] = _sha(C.string_at(C.byref(ps._film_desc), C.sizeof(ps._film_desc)))
    out["samples_per_pixel"] = ps.samples_per_pixel
    out["film_name"] = ps.film_name
    return out


def all_hashes(dirpath, ftn):
    from fountain_amd import PbrtScene
    _inputs(dirpath, ftn)
    out = {}
    for name, text in sorted(scene_texts().items()):
        path = os.path.join(dirpath, name + ".pbrt")
        with open(path, "w") as f:
            f.write(text)
        out[name] = descriptor_hashes(PbrtScene(path, ftn))
    return out


@pytest.fixture(scope="module")
def hashes(ftn, tmp_path_factory):
    return all_hashes(str(tmp_path_factory.mktemp("reader_descriptors")), ftn)


def _recorded():
    return json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}      # absent only while --record writes it


@pytest.mark.parametrize("name", sorted(_recorded()))
def test_parsed_descriptors_match_the_recorded_bits(hashes, name):
    want = _recorded()[name]
    got = hashes[name]
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k] == want[k], "%s: %s differs from the recorded descriptor" % (name, k)


def test_every_scene_text_is_recorded():
    assert sorted(_recorded()) == sorted(scene_texts())


if __name__ == "__main__":
    import tempfile
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    from fountain_amd import default_backend
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_reader_descriptors.py --record"
    with tempfile.TemporaryDirectory() as d:
        rec = all_hashes(d, default_backend())
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d scenes" % len(rec))
