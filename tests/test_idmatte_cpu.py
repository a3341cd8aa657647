"""The parts of the ID-matte extension that need no GPU: the host twins of resolve and select against float32 numpy restatements; the ids
of a scene description; MurmurHash3 and the float conversion of the Cryptomatte encoding; ftn_exr_write_channels through a minimal
OpenEXR reader of the test's own (tests/_idmatte_ref.py); the round trip of fountain_amd/idmatte.py's reader and its --select."""
import ctypes as C
import json

import numpy as np
import pytest

from fountain_amd import FountainError, _abi as A
from fountain_amd import idmatte as I

import _idmatte_ref as R

F32 = np.float32
INV = A.FTN_ERR_INVALID_ARGUMENT


def random_tables(n, seed):
    """tables as a render leaves them (whole-number weights, total the sum of the parts), few ids so that weights tie often"""
    rng = np.random.default_rng(seed)
    raw = np.zeros((n, 20), np.uint32)
    f = raw.view(F32)
    for i in range(n):
        k = int(rng.integers(0, 9))
        raw[i, :k] = rng.choice(np.array([0, 1, 2, 3, 5, 8, 13, 0x7fffffff, 0x80000000, 0xffffffff], np.uint32), k, replace=False)
        f[i, 8:8 + k] = rng.integers(1, 5, k)
        f[i, 16] = rng.integers(0, 4) if k == 8 else 0
        f[i, 17] = rng.integers(0, 3)
        raw[i, 19] = k
        f[i, 18] = f[i, 8:16].sum() + f[i, 16] + f[i, 17]
    return raw


@pytest.mark.parametrize("tables", ["synthetic", "random"])
def test_host_resolve_and_select(ftn, tables):
    raw = R.synthetic_tables() if tables == "synthetic" else random_tables(300, 4)
    f = I.fields(raw)
    tied = [len(set(f["weight"][i, :n].tolist())) < n for i, n in enumerate(np.minimum(f["n_used"], 8))]
    assert sum(tied) >= 3                                      # the tables really contain ties in weight
    if tables == "synthetic":
        assert (f["total"] == 0).any() and (f["n_used"] == 0).any() and (f["n_used"] == 8).any()
        assert (f["id"][:, :3] == 0xffffffff).any() and ((f["id"] == 0) & (np.arange(8) < f["n_used"][:, None])).any()
    want = R.resolve_ref(raw)
    got = I.resolve(ftn, raw)
    assert np.array_equal(got, want)
    rk = I.ranks(got)
    assert (np.diff(rk["coverage"], axis=-1) <= 0).all() and not got[f["total"] == 0].any()
    for ids in ([], [0], [3, 1], [0xffffffff, 5, 5, 3], np.unique(want[:, 0:16:2]).tolist()):
        for kw in (dict(), dict(overflow=True), dict(miss=True), dict(overflow=True, miss=True)):
            assert np.array_equal(I.select(ftn, want, ids, **kw).view(np.uint32), R.select_ref(want, ids, **kw).view(np.uint32)), (ids, kw)
    everything = I.select(ftn, want, np.unique(f["id"]).tolist(), overflow=True, miss=True)
    assert np.abs(everything[f["total"] > 0] - 1.0).max() <= 4 * 2.0 ** -24 * 10


def test_prim_ids(ftn):
    b, _, _ = R.textured_floor(ftn)
    d, keep = b.build_desc()
    mat, names = I.prim_ids(b, "material")
    assert mat.dtype == np.uint32 and mat.tolist() == [(0xffffffff if d.prims[i].material < 0 else d.prims[i].material) for i in range(d.n_prims)]
    assert 0xffffffff in mat.tolist() and 0xffffffff not in names and all(n == "material_%d" % i for i, n in names.items())
    shp, names = I.prim_ids(d, "shape")
    want = [int(d.tri_mesh[d.prims[i].shape_index]) if d.prims[i].shape_kind == A.FTN_SHAPE_TRIANGLE else d.n_meshes + d.prims[i].shape_index for i in range(d.n_prims)]
    assert shp.tolist() == want and len(set(want)) == d.n_meshes + d.n_spheres and names[want[-1]] == "shape_%d" % want[-1]
    prim, names = I.prim_ids(b, "primitive")
    assert prim.tolist() == list(range(d.n_prims)) and names[3] == "primitive_3"
    with pytest.raises(ValueError):
        I.prim_ids(b, "object")


def test_murmur_hash_and_float_conversion():
    fox = b"The quick brown fox jumps over the lazy dog"
    for data, seed, want in ((b"", 0, 0), (b"", 1, 0x514e28b7), (b"\xff\xff\xff\xff", 0, 0x76293b50), ("hello".encode("utf-8"), 0, 0x248bfa47),
                             (fox, 0, 0x2e4ff723), (fox, 0x9747b28c, 0x2fa826cd)):
        assert I.murmur3_32(data, seed) == want, (data, seed)
    # exponent 0 (zero, denormals) and 255 (infinities, NaNs): bit 23 is flipped; every other value stays
    for h, want in ((0x00000000, 0x00800000), (0x007fffff, 0x00ffffff), (0x80000001, 0x80800001), (0x7f800000, 0x7f000000), (0x7fc00000, 0x7f400000),
                    (0xffffffff, 0xff7fffff), (0xff800000, 0xff000000), (0x00800000, 0x00800000), (0x7f7fffff, 0x7f7fffff), (0x3f800000, 0x3f800000),
                    (0x248bfa47, 0x248bfa47)):
        assert I.hash_to_float_bits(h) == want, hex(h)
        v = np.array([I.hash_to_float_bits(h)], np.uint32).view(F32)[0]
        assert np.isfinite(v) and abs(v) >= np.finfo(F32).tiny
    assert I.name_bits("hello") == 0x248bfa47


@pytest.mark.parametrize("w,h", [(1, 1), (33, 7)])
def test_exr_write_channels(ftn, tmp_path, w, h):
    rng = np.random.default_rng(w)
    names = ["L01.R", "L.B", "z", "L00.A", "L.R", "A" * 255, "L00.R"]
    planes = {n: rng.standard_normal((h, w)).astype(F32) for n in names}
    # id floats: hashes made safe, among them bit patterns next to the excluded ones
    idbits = np.array([I.hash_to_float_bits(int(v)) for v in rng.integers(0, 2 ** 32, h * w)], np.uint32).reshape(h, w)
    idbits.flat[0] = I.hash_to_float_bits(0x7fc00001)
    planes["L00.R"] = idbits.view(F32)
    attrs = {"cryptomatte/abc1234/name": "L", "cryptomatte/abc1234/manifest": json.dumps({"näme %d" % i: "%08x" % i for i in range(40)}), "empty": ""}
    path = str(tmp_path / "c.exr")
    I.write_channels(path, planes, attrs, ftn)
    got_names, got, got_attrs = R.read_exr_channels(path)
    assert got_names == sorted(names, key=lambda s: s.encode()) and got_names != names
    for n in names:
        assert np.array_equal(got[n].view(np.uint32), planes[n].view(np.uint32)), n
    assert np.isfinite(got["L00.R"]).all()
    for k, v in attrs.items():
        assert got_attrs[k] == ("string", v.encode("utf-8"))
    assert got_attrs["dataWindow"][1] == got_attrs["displayWindow"][1] == np.array([0, 0, w - 1, h - 1], np.int32).tobytes()
    # the package's own reader
    ch, at = I.read_cryptomatte(path)
    assert sorted(ch) == sorted(names) and all(np.array_equal(ch[n].view(np.uint32), planes[n].view(np.uint32)) for n in names)
    assert at == attrs


def test_exr_write_channels_refusals(ftn, tmp_path):
    lib = I._lib(ftn)
    path = tmp_path / "no.exr"
    plane = np.zeros((2, 3), F32)
    strs = lambda *s: (C.c_char_p * len(s))(*[x.encode() if x is not None else None for x in s])
    ptrs = lambda *a: (C.c_void_p * len(a))(*[x.ctypes.data if x is not None else None for x in a])

    def call(path=str(path).encode(), w=3, h=2, n=2, names=strs("a", "b"), planes=ptrs(plane, plane), n_attrs=1, an=strs("k"), av=strs("v")):
        return lib.ftn_exr_write_channels(path, w, h, n, names, planes, n_attrs, an, av)
    assert call() == 0 and path.exists()
    path.unlink()
    for kw in (dict(path=None), dict(names=None), dict(planes=None), dict(an=None), dict(av=None), dict(names=strs("a", None)), dict(planes=ptrs(plane, None)),
               dict(an=strs(None)), dict(av=strs(None)), dict(w=0), dict(h=0), dict(w=-1), dict(n=0), dict(n_attrs=-1),
               dict(names=strs("a", "a")), dict(names=strs("a", "")), dict(names=strs("a", "b" * 256)), dict(an=strs("k" * 256)), dict(an=strs(""))):
        assert call(**kw) == INV, kw
        assert not path.exists()
    assert call(names=strs("a", "b" * 255), an=strs("k" * 255)) == 0 and call(n_attrs=0, an=None, av=None) == 0
    with pytest.raises(FountainError):
        I.write_channels(str(tmp_path / "missing" / "x.exr"), {"a": plane}, None, ftn)
    with pytest.raises(ValueError):
        I.write_channels(str(path), {"a": plane, "b": np.zeros((3, 2), F32)}, None, ftn)


def test_cryptomatte_round_trip_and_select(ftn, tmp_path):
    raw = random_tables(12 * 9, 7).reshape(9, 12, 20)
    resolved = I.resolve(ftn, raw)
    names = {i: "thing_%d" % i for i in (0, 1, 2, 3, 5, 8, 13, 0x7fffffff, 0x80000000)}        # 0xffffffff has no name: it is called id_4294967295
    path = str(tmp_path / "m_crypto.exr")
    I.write_cryptomatte(path, {"CryptoObject": (resolved, names), "CryptoMaterial": (resolved, {})}, ftn)
    got_names, planes, attrs = R.read_exr_channels(path)
    assert len(got_names) == 2 * (3 + 16) and got_names == sorted(got_names)
    key = "cryptomatte/%s/" % ("%08x" % I.murmur3_32(b"CryptoObject"))[:7]
    assert attrs[key + "name"][1] == b"CryptoObject" and attrs[key + "hash"][1] == b"MurmurHash3_32" and attrs[key + "conversion"][1] == b"uint32_to_float32"
    manifest = json.loads(attrs[key + "manifest"][1])
    assert all(manifest[n] == "%08x" % I.name_bits(n) for n in names.values()) and "id_4294967295" in manifest
    rk = I.ranks(resolved)
    for r in range(8):
        cov = planes["CryptoObject%02d.%s" % (r // 2, "GA"[r % 2])]
        idf = planes["CryptoObject%02d.%s" % (r // 2, "RB"[r % 2])]
        assert np.array_equal(cov.view(np.uint32), rk["coverage"][..., r].view(np.uint32)) and np.isfinite(idf).all()
        for i, n in list(names.items()) + [(0xffffffff, "id_4294967295")]:
            at = (rk["id"][..., r] == i) & (cov > 0)
            assert (idf.view(np.uint32)[at] == I.name_bits(n)).all()
        assert not idf.view(np.uint32)[cov == 0].any()
    # --select through the module's command line: the sum of the named ids' coverages, in rank order
    from fountain_amd import read_exr
    out = str(tmp_path / "mask.exr")
    assert I.main([path, "--layer", "CryptoObject", "--select", "thing_3", "thing_13", "id_4294967295", "-o", out]) == 0
    want = I.select(ftn, resolved, [3, 13, 0xffffffff])
    assert np.array_equal(read_exr(out, ftn)[..., 0].view(np.uint32), want.view(np.uint32)) and want.max() > 0
    assert I.main([path, "--layer", "CryptoObject", "--select", "nothing", "-o", out]) == 2
    assert I.main([path, "--layer", "CryptoDepth", "--select", "thing_3", "-o", out]) == 2
    assert I.main([str(tmp_path / "none.exr"), "--layer", "CryptoObject", "--select", "thing_3", "-o", out]) == 2
