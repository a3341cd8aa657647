"""ID mattes (include/fountain_hip_idmatte.h): per pixel, a ranked list of (id, coverage) over exactly the camera samples ftn_render
traces for the same sampler, tiles and film, and its Cryptomatte encoding in a multi-channel OpenEXR file.

  prim_ids(builder_or_desc, kind)                   one id per primitive, and the names of the ids: kind = material | shape | primitive
  render_idmatte(be, builder, cam, res, sampler, ids)   host buffers -> (resolved [H, W, 20] words, raw [H, W, 20] words, stats)
  render_idmatte_torch(scene, cam, film, sampler, ids, out)   continues a float32 CUDA tensor [H, W, 20] (bit patterns) on the current stream
  resolve(be, raw) / resolve_torch(be, raw, out)    tables -> ranks: (id, coverage) x 8 by weight, overflow, miss, total, n_used
  select(be, resolved, ids) / select_torch(...)     the matte of a set of ids
  write_cryptomatte(path, layers, be)               layers: {layer name: (resolved, names)} -> one OpenEXR file
  read_cryptomatte(path)                            the reader of those files: (channels, attributes)
  python -m fountain_amd.idmatte file_crypto.exr --layer CryptoMaterial --select material_3 -o mask.exr

Both layouts are 20 32-bit words per pixel, kept as uint32 arrays; fields(raw) and ranks(resolved) give typed views.  The reference
renders no mattes, so the CPU oracle has no twin of these calls.

The Cryptomatte encoding (specification 1.2.0): a name's id is MurmurHash3_x86_32 of its UTF-8 bytes with seed 0, stored as the float32 of
the same bits, with bit 23 flipped where the exponent field would be 0 or 255 (so no id is a denormal, an infinity or a NaN).  A layer L
has the preview channels L.R, L.G, L.B and L00 ... L03 with R, G, B, A = id and coverage of ranks 2k and 2k + 1; the file's attributes
cryptomatte/<7 hex digits of hash(L)>/{name, hash, conversion, manifest} describe it, the manifest mapping names to 8 hex digits.
"""
import ctypes as C
import json
import struct
import sys

import numpy as np

from . import _abi as A
from ._cli import refuse
from ._nontwin import bind, call_args, check_tensor as _check_tensor, current_stream, ptr, tptr
from .api import Film, FountainError, default_backend

WORDS = A.FTN_IDMATTE_RESOLVED_WORDS
SLOTS = A.FTN_IDMATTE_SLOTS
NULL_MATERIAL = 0xffffffff
LAYERS = {"material": "CryptoMaterial", "shape": "CryptoObject", "primitive": "CryptoPrimitive"}
LEVELS = SLOTS // 2


def _lib(be):
    return bind(be, A.EXTENSIONS["idmatte"])


# ------------------------------------------------------------------ ids
def prim_ids(builder_or_desc, kind):
    """One uint32 id per primitive in insertion order, from the ftn_scene_desc arrays (a SceneBuilder, a PbrtScene, a Scene or the
    ftn_scene_desc itself), and {id: name}.  material: the material index (null: 0xffffffff), names material_<i>; shape: the mesh id of
    a triangle, n_meshes + the sphere index of a sphere, names shape_<i>; primitive: the insertion index, names primitive_<i>."""
    d, keep = builder_or_desc, None
    if hasattr(d, "build_desc"):
        d, keep = d.build_desc()
    elif not isinstance(d, A.ftn_scene_desc):
        d = d.desc
    n = d.n_prims
    prims = np.ctypeslib.as_array(C.cast(d.prims, C.POINTER(C.c_uint32)), (n, 4)) if n else np.zeros((0, 4), np.uint32)
    if kind == "material":
        ids = prims[:, 2].copy()                    # int32 -1 (no material) reads as 0xffffffff
        ids[prims[:, 2].view(np.int32) < 0] = NULL_MATERIAL
    elif kind == "shape":
        tri_mesh = np.ctypeslib.as_array(d.tri_mesh, (d.n_triangles,)) if d.n_triangles else np.zeros(1, np.uint32)
        is_tri = prims[:, 0] == A.FTN_SHAPE_TRIANGLE
        ids = np.where(is_tri, tri_mesh[np.where(is_tri, prims[:, 1], 0)], np.uint32(d.n_meshes) + prims[:, 1])
    elif kind == "primitive":
        ids = np.arange(n, dtype=np.uint32)
    else:
        raise ValueError("kind must be material, shape or primitive, not %r" % (kind,))
    ids = np.ascontiguousarray(ids, np.uint32)
    names = {int(i): "%s_%d" % (kind, i) for i in np.unique(ids) if int(i) != NULL_MATERIAL or kind != "material"}
    del keep
    return ids, names


# ------------------------------------------------------------------ views
def fields(raw):
    """typed views of raw tables [..., 20]: id [..., 8] uint32, weight [..., 8], overflow, miss, total (float32), n_used (uint32)"""
    raw = np.asarray(raw)
    f = raw.view(np.float32)
    return dict(id=raw[..., 0:8], weight=f[..., 8:16], overflow=f[..., 16], miss=f[..., 17], total=f[..., 18], n_used=raw[..., 19])


def ranks(resolved):
    """typed views of resolved pixels [..., 20]: id [..., 8] uint32 and coverage [..., 8] by rank, overflow, miss, total, n_used (float32)"""
    r = np.asarray(resolved)
    f = r.view(np.float32)
    return dict(id=r[..., 0:16:2], coverage=f[..., 1:16:2], overflow=f[..., 16], miss=f[..., 17], total=f[..., 18], n_used=f[..., 19])


def _words(a, what):
    a = np.ascontiguousarray(a)
    if a.dtype != np.uint32 or a.ndim < 1 or a.shape[-1] != WORDS:
        raise ValueError("%s must be a uint32 array of shape [..., %d]" % (what, WORDS))
    return a


def _id_list(ids):
    ids = np.ascontiguousarray(np.asarray(list(ids) if not isinstance(ids, np.ndarray) else ids, dtype=np.uint64).astype(np.uint32))
    return ids, (ptr(ids) if ids.size else None)


# ------------------------------------------------------------------ the calls
def resolve(be, raw):
    """ftn_idmatte_resolve: tables [..., 20] -> ranked pixels [..., 20] (uint32 words; ranks() gives typed views)"""
    lib = _lib(be)
    raw = _words(raw, "raw")
    out = np.empty(raw.shape, np.uint32)
    be.check(lib.ftn_idmatte_resolve(ptr(raw), raw.size // WORDS, ptr(out)))
    return out


def select(be, resolved, ids, overflow=False, miss=False):
    """ftn_idmatte_select: the matte [...] (float32) of the ids in `ids` over ranked pixels [..., 20]"""
    lib = _lib(be)
    r = _words(resolved, "resolved")
    ids, p = _id_list(ids)
    out = np.empty(r.shape[:-1], np.float32)
    flags = (A.FTN_IDMATTE_SELECT_OVERFLOW if overflow else 0) | (A.FTN_IDMATTE_SELECT_MISS if miss else 0)
    be.check(lib.ftn_idmatte_select(ptr(r), r.size // WORDS, p, ids.size, flags, ptr(out)))
    return out


def render_idmatte(be, builder, cam, res, sampler, ids, tiles=None, crop=(0.0, 0.0, 1.0, 1.0), scene=None, raw=None,
                   pipeline=A.FTN_PIPELINE_AUTO, device=-1, film=None):
    """Shaped like render_gbuffer: create_scene (unless `scene` is given) + Film (unless `film` is given) + ftn_render_idmatte with one
    id per primitive (prim_ids).  `raw` ([H, W, 20] uint32) is continued when given, else an empty buffer is.  Returns (resolved, raw,
    stats)."""
    lib = _lib(be)
    scene = scene or builder.create_scene()
    film = film or Film(be, res, crop)
    if raw is None:
        raw = np.zeros((film.height, film.width, WORDS), np.uint32)
    if raw.shape != (film.height, film.width, WORDS) or raw.dtype != np.uint32 or not raw.flags.c_contiguous:
        raise ValueError("raw must be a C-contiguous uint32 array of shape %r" % ((film.height, film.width, WORDS),))
    ids = np.ascontiguousarray(ids, np.uint32)
    args, keep = call_args(cam, film, None, sampler, tiles, pipeline, device)
    st = A.ftn_stats()
    be.check(lib.ftn_render_idmatte(scene.handle, *args, ptr(ids), ids.size, ptr(raw), C.byref(st)))
    return resolve(be, raw), raw, st.as_dict()


def render_idmatte_torch(scene, cam, film, sampler, ids, out, tiles=None, pipeline=A.FTN_PIPELINE_AUTO):
    """ftn_render_idmatte_device into `out` (float32 CUDA tensor [H, W, 20] holding the tables' bit patterns, continued) on the current
    stream of its device."""
    be = scene.be
    lib = _lib(be)
    _check_tensor(out, (film.height, film.width, WORDS))
    ids = np.ascontiguousarray(ids, np.uint32)
    args, keep = call_args(cam, film, None, sampler, tiles, pipeline, out.device.index)
    st = A.ftn_stats()
    be.check(lib.ftn_render_idmatte_device(scene.handle, *args, ptr(ids), ids.size, tptr(out), C.c_void_p(current_stream(out)), C.byref(st)))
    return st.as_dict()


def resolve_torch(be, raw, out):
    """ftn_idmatte_resolve_device: raw [..., 20] -> out [..., 20], both float32 CUDA tensors of bit patterns, current stream"""
    lib = _lib(be)
    _check_tensor(raw, raw.shape)
    _check_tensor(out, raw.shape)
    if raw.shape[-1] != WORDS:
        raise ValueError("the last dimension holds the 20 words of a pixel")
    be.check(lib.ftn_idmatte_resolve_device(tptr(raw), raw.numel() // WORDS, tptr(out), C.c_void_p(current_stream(raw))))
    return out


def select_torch(be, resolved, ids, out, overflow=False, miss=False):
    """ftn_idmatte_select_device: resolved [..., 20] -> out [...], float32 CUDA tensors, current stream"""
    lib = _lib(be)
    _check_tensor(resolved, resolved.shape)
    _check_tensor(out, resolved.shape[:-1])
    if resolved.shape[-1] != WORDS:
        raise ValueError("the last dimension holds the 20 words of a pixel")
    ids, p = _id_list(ids)
    flags = (A.FTN_IDMATTE_SELECT_OVERFLOW if overflow else 0) | (A.FTN_IDMATTE_SELECT_MISS if miss else 0)
    be.check(lib.ftn_idmatte_select_device(tptr(resolved), resolved.numel() // WORDS, p, ids.size, flags, tptr(out),
                                           C.c_void_p(current_stream(resolved))))
    return out


# ------------------------------------------------------------------ the Cryptomatte encoding
def murmur3_32(data, seed=0):
    """MurmurHash3_x86_32 of a bytes object"""
    M = 0xffffffff
    rotl = lambda x, r: ((x << r) | (x >> (32 - r))) & M
    h = seed & M
    n = len(data)
    for i in range(0, n - n % 4, 4):
        k = struct.unpack_from("<I", data, i)[0]
        k = (rotl((k * 0xcc9e2d51) & M, 15) * 0x1b873593) & M
        h = (rotl(h ^ k, 13) * 5 + 0xe6546b64) & M
    tail = data[n - n % 4:]
    if tail:
        k = int.from_bytes(tail, "little")
        h ^= (rotl((k * 0xcc9e2d51) & M, 15) * 0x1b873593) & M
    h ^= n
    h ^= h >> 16
    h = (h * 0x85ebca6b) & M
    h ^= h >> 13
    h = (h * 0xc2b2ae35) & M
    return h ^ (h >> 16)


def hash_to_float_bits(h):
    """the bits of the float32 a hash is stored as: bit 23 flipped where the exponent field is 0 or 255"""
    return h ^ (1 << 23) if ((h >> 23) & 255) in (0, 255) else h


def name_bits(name):
    """the bits of the float32 id of a name"""
    return hash_to_float_bits(murmur3_32(name.encode("utf-8")))


def layer_planes(layer, resolved, names):
    """The channels of one layer: {channel name: [H, W] float32} and its manifest {name: bits}.  An id without a name is called
    id_<id>; ranks without coverage hold id 0.0."""
    rk = ranks(_words(resolved, "resolved"))
    if rk["id"].ndim != 3:
        raise ValueError("resolved must be [H, W, 20]")
    used = rk["coverage"] > 0
    manifest = {n: name_bits(n) for n in names.values()}
    table = {}
    for i in np.unique(rk["id"][used]):
        name = names.get(int(i), "id_%d" % int(i))
        table[int(i)] = manifest.setdefault(name, name_bits(name))
    bits = np.zeros(rk["id"].shape, np.uint32)
    for i, b in table.items():
        bits[used & (rk["id"] == np.uint32(i))] = b
    cov = np.where(used, rk["coverage"], np.float32(0)).astype(np.float32)
    planes = {}
    for lv in range(LEVELS):
        for ch, a in zip("RGBA", (bits[..., 2 * lv].view(np.float32), cov[..., 2 * lv], bits[..., 2 * lv + 1].view(np.float32), cov[..., 2 * lv + 1])):
            planes["%s%02d.%s" % (layer, lv, ch)] = np.ascontiguousarray(a, np.float32)
    # the preview: two colours taken from the bits of the first rank's id, scaled by its coverage
    b0 = bits[..., 0].astype(np.uint64)
    planes[layer + ".R"] = np.zeros(cov.shape[:2], np.float32)
    planes[layer + ".G"] = (((b0 << 8) & 0xffffffff).astype(np.float64) / 2.0 ** 32 * cov[..., 0]).astype(np.float32)
    planes[layer + ".B"] = (((b0 << 16) & 0xffffffff).astype(np.float64) / 2.0 ** 32 * cov[..., 0]).astype(np.float32)
    return planes, manifest


def write_channels(path, planes, attrs=None, be=None):
    """ftn_exr_write_channels: {channel name: [H, W] float32} and {attribute name: string}"""
    be = be or default_backend()
    lib = _lib(be)
    names = list(planes)
    arrs = [np.ascontiguousarray(planes[n], np.float32) for n in names]
    if not arrs or any(a.ndim != 2 or a.shape != arrs[0].shape for a in arrs):
        raise ValueError("planes must be [H, W] arrays of one size")
    attrs = attrs or {}
    strings = lambda items: (C.c_char_p * max(len(items), 1))(*[s.encode("utf-8") for s in items])
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    h, w = arrs[0].shape
    rc = lib.ftn_exr_write_channels(path.encode(), w, h, len(arrs), strings(names), ptrs, len(attrs), strings(list(attrs)), strings(list(attrs.values())))
    if rc != 0:
        raise FountainError(rc, be.lib.ftn_imageio_last_error().decode(errors="replace"))


def write_cryptomatte(path, layers, be=None):
    """layers: {layer name: (resolved [H, W, 20], names {id: name})} -> one OpenEXR file with every layer's channels and attributes"""
    planes, attrs = {}, {}
    for layer, (resolved, names) in layers.items():
        p, manifest = layer_planes(layer, resolved, names)
        planes.update(p)
        key = "cryptomatte/%s/" % ("%08x" % murmur3_32(layer.encode("utf-8")))[:7]
        attrs[key + "name"] = layer
        attrs[key + "hash"] = "MurmurHash3_32"
        attrs[key + "conversion"] = "uint32_to_float32"
        attrs[key + "manifest"] = json.dumps({n: "%08x" % b for n, b in sorted(manifest.items())}, separators=(",", ":"))
    write_channels(path, planes, attrs, be)


def read_cryptomatte(path):
    """The reader of write_channels' files (scanline, uncompressed, FLOAT channels): ({channel: [H, W] float32}, {attribute: string})"""
    buf = open(path, "rb").read()
    if len(buf) < 8 or buf[:4] != b"\x76\x2f\x31\x01" or buf[5] & 0x1a:
        raise ValueError("%s: not a scanline OpenEXR file" % path)
    p, attrs, chans, dw, compression = 8, {}, [], None, None

    def cstr(at):
        end = buf.index(b"\0", at)
        return buf[at:end].decode("utf-8"), end + 1
    while buf[p] != 0:
        name, p = cstr(p)
        typ, p = cstr(p)
        size = struct.unpack_from("<i", buf, p)[0]
        data, p = buf[p + 4:p + 4 + size], p + 4 + size
        if typ == "string":
            attrs[name] = data.decode("utf-8")
        elif name == "channels":
            q = 0
            while data[q] != 0:
                end = data.index(b"\0", q)
                chans.append((data[q:end].decode("utf-8"), struct.unpack_from("<i", data, end + 1)[0]))
                q = end + 17
        elif name == "dataWindow":
            dw = struct.unpack("<4i", data)
        elif name == "compression":
            compression = data[0]
    if dw is None or compression != 0 or not chans or any(t != 2 for _, t in chans):
        raise ValueError("%s: only uncompressed files of FLOAT channels, as this package writes them, are read" % path)
    p += 1
    w, h = dw[2] - dw[0] + 1, dw[3] - dw[1] + 1
    out = {n: np.empty((h, w), np.float32) for n, _ in chans}
    for off in struct.unpack_from("<%dQ" % h, buf, p):
        y, nbytes = struct.unpack_from("<2i", buf, off)
        if nbytes != 4 * w * len(chans) or not dw[1] <= y <= dw[3]:
            raise ValueError("%s: corrupt scanline" % path)
        row = np.frombuffer(buf, np.float32, w * len(chans), off + 8).reshape(len(chans), w)
        for k, (n, _) in enumerate(chans):
            out[n][y - dw[1]] = row[k]
    return out, attrs


def file_select(path, layer, names, be=None):
    """the matte [H, W] of the named ids of one layer of a file of write_cryptomatte.  Names the manifest does not hold are an error.
    (Overflow and miss shares are not stored in the file: a pixel's ranks simply do not sum to one where there were any.)"""
    be = be or default_backend()
    chans, attrs = read_cryptomatte(path)
    keys = [k[:-4] for k, v in attrs.items() if k.startswith("cryptomatte/") and k.endswith("/name") and v == layer]
    if not keys:
        raise ValueError("%s has no Cryptomatte layer %s" % (path, layer))
    manifest = json.loads(attrs[keys[0] + "manifest"])
    missing = [n for n in names if n not in manifest]
    if missing:
        raise ValueError("layer %s has no id named %s" % (layer, ", ".join(missing)))
    first = chans["%s00.R" % layer]
    r = np.zeros(first.shape + (WORDS,), np.uint32)
    for lv in range(LEVELS):
        for k, ch in enumerate("RGBA"):
            r[..., 4 * lv + k] = chans["%s%02d.%s" % (layer, lv, ch)].view(np.uint32)
    return select(be, r, [int(manifest[n], 16) for n in names])


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="fountain_amd.idmatte")
    ap.add_argument("file")
    ap.add_argument("--layer", required=True)
    ap.add_argument("--select", nargs="+", required=True, metavar="NAME")
    ap.add_argument("-o", "--output", required=True)
    opts = ap.parse_args(argv)
    from .api import write_exr
    be = default_backend()
    try:
        mask = file_select(opts.file, opts.layer, opts.select, be=be)
    except (OSError, ValueError, KeyError) as e:
        return refuse(e)
    write_exr(opts.output, np.repeat(mask[..., None], 3, axis=-1), be)
    return 0


if __name__ == "__main__":
    sys.exit(main())
