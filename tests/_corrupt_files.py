"""A catalogue of corrupt PBRT, PLY and OpenEXR files, and the walker that feeds them to ftn_pbrt_load, ftn_ply_load and ftn_exr_read.

Seeds are made here (pure Python, plus the library's own EXR writer for the uncompressed FLOAT variant); nothing is fetched or committed.
Every mutation is deterministic and has a name, which is what a failure reports.  A *family* is one (reader, seed) pair: its cases are
walked by one fresh child process (`--walk`, started by test_corrupt_files.py) which appends each case's name to a progress file before
the call, so that a crash or a hang names its case.  `--write DIR` writes every file and a manifest for tools/reader_check.cpp.

The contract a case is held to (check_* below):
  * the call returns, with FTN_OK or one of INVALID_ARGUMENT / UNSUPPORTED / OUT_OF_MEMORY, and a refusal leaves a message;
  * a case marked must_refuse (every strict prefix of a binary seed among them) is refused;
  * an accepted file gave outputs consistent with what it says: every element written (the arrays are pre-filled with a NaN payload),
    PLY indices below the vertex count, PLY triangles equal to the seed's wherever the mutation did not touch them, the EXR size equal
    to the data window;
  * after a refusal the untouched seed still reads back with the seed's bits.
"""
import ctypes as C
import json
import os
import struct
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

FTN_OK, INVALID_ARGUMENT, OUT_OF_MEMORY, UNSUPPORTED = 0, -1, -3, -5
ALLOWED = (FTN_OK, INVALID_ARGUMENT, UNSUPPORTED, OUT_OF_MEMORY)
VALUES = [0, 1, -1, -2 ** 31, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 64 - 4]       # what every 32- / 64-bit field is set to
BYTES = [0x00, 0x7f, 0x80, 0xff]                                                  # what every header byte is set to
N_RANDOM = 2000                                                                   # seeded single-byte changes per seed
SENTINEL = 0x7fc0dead                                                             # a NaN no reader here produces


def case(name, data, **kw):
    c = dict(name=name, data=data, must_refuse=False, random=False)
    c.update(kw)
    return c


def _set(b, off, payload):
    return b[:off] + payload + b[off + len(payload):]


def _field(v, nbytes):
    return (v & ((1 << (8 * nbytes)) - 1)).to_bytes(nbytes, "little")


def random_byte_cases(seed_bytes, rng_seed, n=N_RANDOM):
    rng = np.random.default_rng(rng_seed)
    pos = rng.integers(0, len(seed_bytes), n)
    val = rng.integers(1, 256, n)                                  # added to the old byte mod 256: always a change
    for k in range(n):
        p = int(pos[k]); v = (seed_bytes[p] + int(val[k])) & 255
        yield p, v, case("random %d: byte %d = 0x%02x" % (k, p, v), _set(seed_bytes, p, bytes([v])), random=True)


# ------------------------------------------------------------------ OpenEXR: packers (the encoders test_output_stage.py checks the reader with)
EXR_MAGIC = bytes([0x76, 0x2f, 0x31, 0x01, 2, 0, 0, 0])


def exr_predict(raw):
    """The two-halves de-interleave and the byte delta predictor OpenEXR applies before RLE and ZIP."""
    n = len(raw)
    t = bytes(raw[0::2]) + bytes(raw[1::2])
    d = bytearray(n); d[0] = t[0]
    for i in range(1, n):
        d[i] = (t[i] - t[i - 1] + 128) & 255
    return bytes(d)


def rle_block(raw):
    """OpenEXR RLE: de-interleave into two halves, delta-predict, then run-length encode (runs as literals here and there)."""
    n = len(raw)
    d = exr_predict(raw)
    out, i = bytearray(), 0
    while i < n:
        j = i
        while j + 1 < n and d[j + 1] == d[i] and j - i < 126:
            j += 1
        if j - i >= 2:
            out += struct.pack("b", j - i) + bytes([d[i]]); i = j + 1
        else:
            k = i
            while k < n and k - i < 127 and not (k + 2 < n and d[k] == d[k + 1] == d[k + 2]):
                k += 1
            out += struct.pack("b", -(k - i)) + bytes(d[i:k]); i = k
    return bytes(out)


def zip_block(raw):
    return zlib.compress(exr_predict(raw))


def exr_attr(name, typ, data):
    return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(data)) + data


def exr_attrs(w, h, comp, half=False):
    chl = b"".join(c.encode() + b"\0" + struct.pack("<iB3xii", 1 if half else 2, 0, 1, 1) for c in "BGR") + b"\0"
    box = struct.pack("<4i", 0, 0, w - 1, h - 1)
    return [["channels", "chlist", chl], ["compression", "compression", bytes([comp])], ["dataWindow", "box2i", box], ["displayWindow", "box2i", box],
            ["lineOrder", "lineOrder", b"\0"], ["pixelAspectRatio", "float", struct.pack("<f", 1)], ["screenWindowCenter", "v2f", struct.pack("<2f", 0, 0)],
            ["screenWindowWidth", "float", struct.pack("<f", 1)]]


def exr_assemble(attrs, blocks):
    """attrs: (name, type, data); blocks: (y, data), stored in this order with the offset table naming their places."""
    hdr = EXR_MAGIC + b"".join(exr_attr(*a) for a in attrs) + b"\0"
    off, offs = len(hdr) + 8 * len(blocks), []
    for y, data in blocks:
        offs.append(off); off += 8 + len(data)
    return hdr + b"".join(_field(o, 8) for o in offs) + b"".join(struct.pack("<ii", y, len(d)) + d for y, d in blocks)


def exr_blocks(img, comp, half=False):
    h, w = img.shape[:2]
    lines = 16 if comp == 3 else 1
    blocks = []
    for y0 in range(0, h, lines):
        raw = b"".join(img[y, :, "RGB".index(c)].astype("<f2" if half else "<f4").tobytes() for y in range(y0, min(y0 + lines, h)) for c in "BGR")
        packed = raw if comp == 0 else rle_block(raw) if comp == 1 else zip_block(raw)
        blocks.append((y0, packed if len(packed) < len(raw) else raw))          # OpenEXR stores the raw block when compression does not help
    return blocks


def exr_file(img, comp, half=False):
    """A scanline OpenEXR file of img [h, w, 3] float32: comp 0 none, 1 RLE, 2 ZIPS (one line a block), 3 ZIP (16 lines a block); B G R channels."""
    h, w = img.shape[:2]
    return exr_assemble(exr_attrs(w, h, comp, half), exr_blocks(img, comp, half))


def exr_parse(b):
    """(attrs, offsets, blocks, layout) of a well-formed file; layout names the places of its 32- and 64-bit fields and of its attributes."""
    p, attrs, f32, where = 8, [], [("version", 4)], []
    while b[p] != 0:
        e = b.index(0, p); name = b[p:e].decode(); p = e + 1
        e = b.index(0, p); typ = b[p:e].decode(); p = e + 1
        (n,) = struct.unpack_from("<i", b, p)
        f32.append((name + ".size", p)); where.append((name, p, n)); p += 4
        data = b[p:p + n]
        if typ == "chlist":
            q = 0
            while data[q] != 0:
                e = data.index(0, q); ch = data[q:e].decode(); q = e + 1
                f32 += [("%s.%s.%s" % (name, ch, fld), p + q + 4 * k) for k, fld in enumerate(("type", "pLinear", "xSampling", "ySampling"))]; q += 16
        elif typ in ("box2i", "float", "v2f"):
            f32 += [("%s[%d]" % (name, k), p + 4 * k) for k in range(n // 4)]
        attrs.append([name, typ, data]); p += n
    p += 1
    a = {x[0]: x[2] for x in attrs}
    x0, y0, x1, y1 = struct.unpack("<4i", a["dataWindow"])
    lines = 16 if a["compression"][0] == 3 else 1
    nb = (y1 - y0 + 1 + lines - 1) // lines
    offs = list(struct.unpack_from("<%dQ" % nb, b, p))
    f64 = [("offset[%d]" % k, p + 8 * k) for k in range(nb)]
    blocks = []
    for k, o in enumerate(offs):
        y, n = struct.unpack_from("<ii", b, o)
        f32 += [("block[%d].y" % k, o), ("block[%d].size" % k, o + 4)]
        blocks.append((y, b[o + 8:o + 8 + n]))
    return attrs, offs, blocks, dict(f32=f32, f64=f64, attrs=where, header_end=p, table=p, n_blocks=nb)


def exr_window(b):
    """(w, h) of the last dataWindow attribute, read with every bound checked; None where the header cannot be walked."""
    try:
        p, dw = 8, None
        if len(b) < 8:
            return None
        while True:
            e = b.index(0, p); name = b[p:e]; p = e + 1
            if not name:
                break
            e = b.index(0, p); p = e + 1
            (n,) = struct.unpack_from("<i", b, p); p += 4
            if n < 0 or p + n > len(b):
                return None
            if name == b"dataWindow":
                if n != 16:
                    return None
                dw = struct.unpack_from("<4i", b, p)
            p += n
        return None if dw is None else (dw[2] - dw[0] + 1, dw[3] - dw[1] + 1)
    except (ValueError, struct.error):
        return None


def exr_image(w, h):
    """Values in (0, 1) with runs and repeats, so that the RLE, ZIPS and ZIP blocks of even a 4 x 3 image are stored packed."""
    rng = np.random.default_rng(100 * w + h)
    img = np.full((h, w, 3), 0.25, np.float32)
    img[:, 0] = rng.integers(1, 8, (h, 3)).astype(np.float32) / np.float32(8)
    img[h // 2, w // 2] = (0.5, 0.75, 0.125)
    return img


EXR_VARIANTS = {"float": (0, False), "rle": (1, False), "zips": (2, False), "zip": (3, False), "half": (1, True)}
EXR_SIZES = [(4, 3), (5, 17)]


def exr_seed(variant, w, h, lib_write_exr):
    comp, half = EXR_VARIANTS[variant]
    img = exr_image(w, h)
    if half:
        img = img.astype(np.float16).astype(np.float32)
    return lib_write_exr(img) if variant == "float" else exr_file(img, comp, half)


def exr_cases(seed, rng_seed):
    attrs, offs, blocks, lay = exr_parse(seed)
    for n in range(len(seed)):
        yield case("prefix of %d bytes" % n, seed[:n], must_refuse=True)
    for name, off in lay["f32"]:
        for v in VALUES:
            yield case("%s = %d" % (name, v), _set(seed, off, _field(v, 4)))
    for name, off in lay["f64"]:
        for v in VALUES:
            yield case("%s = %d" % (name, v), _set(seed, off, _field(v, 8)))
    for off in range(lay["header_end"]):
        for v in BYTES:
            if seed[off] != v:
                yield case("header byte %d = 0x%02x" % (off, v), _set(seed, off, bytes([v])))
    for name, off, n in lay["attrs"]:
        for what, v in (("0", 0), ("size-1", n - 1), ("past the end of the file", len(seed))):
            yield case("%s: size field says %s" % (name, what), _set(seed, off, _field(v, 4)))
    # attributes that really are shorter: the header still parses, the reader must not read what is not there
    for name in ("channels", "compression", "dataWindow", "lineOrder"):
        for cut in ("0", "size-1"):
            aa = [[a[0], a[1], b"" if a[0] == name and cut == "0" else a[2][:-1] if a[0] == name else a[2]] for a in attrs]
            yield case("%s attribute of size %s" % (name, cut), exr_assemble(aa, blocks), must_refuse=name != "lineOrder" or cut == "0")
    aa = [[a[0], a[1], b"RR" if a[0] == "channels" else a[2]] for a in attrs]
    yield case("channels attribute of size 2 holding RR", exr_assemble(aa, blocks), must_refuse=True)
    # the same attributes as the last bytes of the file: what a reader takes from them without looking at their size lies past the end
    for name, typ, data in (("channels", "chlist", b"RR"), ("dataWindow", "box2i", b""), ("compression", "compression", b""), ("lineOrder", "lineOrder", b"")):
        yield case("file that ends in a %s attribute of size %d" % (name, len(data)), EXR_MAGIC + exr_attr(name, typ, data), must_refuse=True)
    for what, box in (("0..0x7ffffffe", (0, 0, 0x7ffffffe, 0x7ffffffe)), ("of width 2^32", (-2 ** 31, 0, 2 ** 31 - 1, 0)), ("of height 2^32", (0, -2 ** 31, 0, 2 ** 31 - 1)),
                      ("of width 2^28 + 1", (0, 0, 2 ** 28, 0))):
        aa = [[a[0], a[1], struct.pack("<4i", *box) if a[0] == "dataWindow" else a[2]] for a in attrs]
        yield case("dataWindow " + what, exr_assemble(aa, blocks), must_refuse=True)
    yield case("first scanline offset 2^64-4", _set(seed, lay["table"], _field(2 ** 64 - 4, 8)), must_refuse=True)
    nb = lay["n_blocks"]
    if nb > 1:
        same = dict(same_pixels=True)
        yield case("offset table reversed", _set(seed, lay["table"], b"".join(_field(o, 8) for o in offs[::-1])), **same)
        yield case("offset table rotated", _set(seed, lay["table"], b"".join(_field(o, 8) for o in offs[1:] + offs[:1])), **same)
        yield case("blocks stored in reverse order", exr_assemble(attrs, blocks[::-1]), **same)
        yield case("offset table with two equal entries", _set(seed, lay["table"] + 8, _field(offs[0], 8)), must_refuse=True)
        yield case("two blocks with the same y", exr_assemble(attrs, [blocks[0], (blocks[0][0], blocks[1][1])] + blocks[2:]), must_refuse=True)
        yield case("one block short", exr_assemble(attrs, blocks[:-1]), must_refuse=True)
    for p, v, c in random_byte_cases(seed, rng_seed):
        yield c


# ------------------------------------------------------------------ PLY
PLY_CODE = {"uchar": "B", "uint8": "B", "char": "b", "ushort": "H", "short": "h", "int": "i", "int32": "i", "uint": "I", "float": "f"}
PLY_P = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0.5, 0.5, 1)]
PLY_N = [(0, 0, -1), (0.5, 0, -0.5), (0.5, 0.5, -0.5), (0, 0.5, -0.5), (0, 0, 1)]
PLY_UV = [(0, 0), (1, 0), (1, 1), (0, 1), (0.5, 0.5)]
PLY_F = [(0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4)]


def _pack_int(code, v):
    size = struct.calcsize(code)
    return _field(int(v), size)


def ply_file(F=PLY_F, normals=False, binary=True, cnt_t="uchar", idx_t="int", nv=None, nf=None, eol="\n", end_header=True, vertex_list=False):
    """-> (bytes, layout): layout has header_len and, for a binary file, the byte range of every vertex field and face record."""
    cols = [PLY_P] + ([PLY_N, PLY_UV] if normals else [])
    rows = [[x for c in cols for x in c[i]] for i in range(len(PLY_P))]
    props = ["x", "y", "z"] + (["nx", "ny", "nz", "u", "v"] if normals else [])
    hdr = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "comment made by tests/_corrupt_files.py",
           "element vertex %d" % (len(PLY_P) if nv is None else nv)] + ["property float %s" % p for p in props]
    if vertex_list:
        hdr.append("property list uchar int neighbours")
    hdr += ["element face %d" % (len(F) if nf is None else nf), "property list %s %s vertex_indices" % (cnt_t, idx_t)] + (["end_header"] if end_header else [])
    head = "".join(h + eol for h in hdr).encode()
    lay = dict(header_len=len(head), f32=[], faces=[])
    if not binary:
        body = "".join(" ".join(repr(float(x)) for x in r) + "\n" for r in rows) + "".join("3 %d %d %d\n" % tuple(t) for t in F)
        return head + body.encode(), lay
    body = b""
    for i, r in enumerate(rows):
        lay["f32"] += [("vertex[%d].%s" % (i, props[k]), len(head) + len(body) + 4 * k, None) for k in range(len(r))]
        body += struct.pack("<%df" % len(r), *r)
    cs, isz = struct.calcsize(PLY_CODE[cnt_t]), struct.calcsize(PLY_CODE[idx_t])
    for t, tri in enumerate(F):
        o = len(head) + len(body)
        if cs == 4:
            lay["f32"].append(("face[%d].count" % t, o, t))
        if isz == 4:
            lay["f32"] += [("face[%d].index[%d]" % (t, k), o + cs + 4 * k, t) for k in range(3)]
        body += _pack_int(PLY_CODE[cnt_t], 3) + b"".join(_pack_int(PLY_CODE[idx_t], v) for v in tri)
        lay["faces"].append((o, len(head) + len(body)))
    return head + body, lay


def ply_families():
    return [("ply-%s-%s-%s" % ("binary" if b else "ascii", "normals-uv" if n else "positions", c), dict(binary=b, normals=n, cnt_t=c))
            for b in (True, False) for n in (False, True) for c in ("uchar", "int")]


def ply_cases(kw, rng_seed):
    seed, lay = ply_file(**kw)
    binary, nf, nv, all_tris = kw["binary"], len(PLY_F), len(PLY_P), list(range(len(PLY_F)))
    body_kw = lambda touched: dict(tris=[t for t in all_tris if t != touched], counts=(nv, nf))
    if binary:
        for n in range(len(seed)):
            yield case("prefix of %d bytes" % n, seed[:n], must_refuse=True)
        yield case("cut 5 bytes into its last face", seed[:lay["faces"][-1][0] + 5], must_refuse=True)
        for name, off, tri in lay["f32"]:
            for v in VALUES:
                yield case("%s = %d" % (name, v), _set(seed, off, _field(v, 4)), **body_kw(tri))
    for off in range(lay["header_len"]):
        for v in BYTES:
            if seed[off] != v:
                yield case("header byte %d = 0x%02x" % (off, v), _set(seed, off, bytes([v])))
    for n in (0, nv - 1, nv + 1, 10 ** 14, 99999999999999):
        yield case("element vertex %d" % n, ply_file(nv=n, **kw)[0], must_refuse=n > nv + 1)
    for n in (0, nf - 1, nf + 1, 10 ** 14):
        yield case("element face %d" % n, ply_file(nf=n, **kw)[0], must_refuse=n > nf, **(dict(tris=list(range(n)), counts=(nv, n)) if n < nf else {}))
    for v in (-1, nv, 2 ** 31):
        for t, k in ((0, 0), (nf - 1, 2)):
            F = [tuple(v if (a, b) == (t, k) else x for b, x in enumerate(tri)) for a, tri in enumerate(PLY_F)]
            yield case("face[%d].index[%d] is %d" % (t, k, v), ply_file(F=F, **kw)[0], must_refuse=True)
    for ty in ("ushort", "uchar", "short"):
        # a correct file of that type: the binary reader decodes 4-byte indices and 1- or 4-byte counts only, an ASCII file is numbers
        k2 = dict(kw, idx_t=ty)
        yield case("index type " + ty, ply_file(**k2)[0], must_refuse=binary, tris=all_tris, counts=(nv, nf))
        k2 = dict(kw, cnt_t=ty)
        yield case("count type " + ty, ply_file(**k2)[0], must_refuse=binary and ty != "uchar", tris=all_tris, counts=(nv, nf))
    yield case("property list inside element vertex", ply_file(vertex_list=True, **kw)[0], must_refuse=True)
    yield case("CRLF header", ply_file(eol="\r\n", **kw)[0], tris=all_tris, counts=(nv, nf))
    yield case("no end_header", ply_file(end_header=False, **kw)[0], must_refuse=True)
    for p, v, c in random_byte_cases(seed, rng_seed):
        if binary and p >= lay["header_len"]:
            hit = [t for t, (a, b) in enumerate(lay["faces"]) if a <= p < b]
            c.update(body_kw(hit[0] if hit else None))
        yield c


# ------------------------------------------------------------------ PBRT: a case is a directory of files, s.pbrt the one that is loaded
def pbrt_seed():
    from test_pbrt_loader import FEATURES, INC
    return {"s.pbrt": FEATURES.encode(), "inc.pbrt": INC.encode(), "cube.ply": ply_file(normals=True)[0]}


WORLD = 'Camera "perspective"\nWorldBegin\n%s\nWorldEnd\n'
WORLD_STATE = ['AttributeBegin', 'AttributeEnd', 'TransformBegin', 'TransformEnd', 'ReverseOrientation', 'Material "matte"', 'Material "matte" "texture Kd" "t"',
               'Material "matte" "texture Kd" []', 'NamedMaterial "gold"', 'MakeNamedMaterial "m" "string type" "matte"', 'AreaLightSource "diffuse"',
               'LightSource "point"', 'LightSource "infinite"', 'Shape "sphere"', 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 0 1 0]',
               'Texture "t" "spectrum" "uv"', 'ObjectInstance "a"', 'WorldEnd']
TRI = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 0 1 0]'
TETRA = 'Shape "loopsubdiv" "integer levels" [%s] "integer indices" [0 1 2 0 3 1 1 3 2 2 3 0] "point P" [0 0 0 1 0 0 0 1 0 0 0 1]'


def grid_mesh(n, bad, every):
    """Shape "trianglemesh": n x n quads over (n + 1)^2 vertices, with `bad` as one coordinate of every `every`-th vertex."""
    P, idx = [], []
    for j in range(n + 1):
        for i in range(n + 1):
            k = j * (n + 1) + i
            c = ["%g" % (0.5 * i), "%g" % (0.25 * j), "%g" % (0.125 * ((7 * i + 3 * j) % 5))]
            if k % every == 0:
                c[k % 3] = bad
            P += c
    for j in range(n):
        for i in range(n):
            v = j * (n + 1) + i
            idx += [v, v + 1, v + n + 2, v, v + n + 2, v + n + 1]
    return 'Shape "trianglemesh" "integer indices" [%s] "point P" [%s]' % (" ".join(str(x) for x in idx), " ".join(P))


def pbrt_cases(rng_seed):
    seed = pbrt_seed()
    one = lambda name, text, **kw: case(name, dict(seed, **{"s.pbrt": text.encode() if isinstance(text, str) else text}), **kw)
    features = seed["s.pbrt"].decode()
    for d in WORLD_STATE:
        yield one("%s before WorldBegin" % d, 'Camera "perspective"\n%s\nWorldBegin\nShape "sphere"\nWorldEnd\n' % d, must_refuse=True)
    yield one("unbalanced AttributeEnd", WORLD % 'AttributeBegin\nAttributeEnd\nAttributeEnd', must_refuse=True)
    yield one("unbalanced TransformEnd", WORLD % 'TransformBegin\nTransformEnd\nTransformEnd', must_refuse=True)
    yield one("AttributeBegin closed by TransformEnd", WORLD % 'AttributeBegin\nTransformEnd\nAttributeEnd\nShape "sphere"', must_refuse=True)
    yield one("AttributeBegin never closed", WORLD % 'AttributeBegin\nTransformBegin\nShape "sphere"')
    yield one("unterminated string", 'Camera "perspective"\nWorldBegin\nShape "sphere\nWorldEnd\n', must_refuse=True)
    yield one("unterminated string in a parameter list", WORLD % 'Shape "sphere" "float radius', must_refuse=True)
    yield one("unterminated bracket", 'Camera "perspective"\nWorldBegin\nShape "trianglemesh" "integer indices" [0 1 2', must_refuse=True)
    yield one("unterminated bracket before more statements", WORLD % 'Shape "trianglemesh" "integer indices" [0 1 2 "point P" [0 0 0 1 0 0 0 1 0]', must_refuse=True)
    yield one("unterminated bracket of a transform", 'Camera "perspective"\nWorldBegin\nTransform [1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 1', must_refuse=True)
    tex = 'Texture "f" "float" "checkerboard" "float tex1" 0 "float tex2" 1\n'
    for where in ('Material "matte" "texture Kd" []', 'Material "matte" "texture sigma" []', 'Texture "c" "spectrum" "checkerboard" "texture tex1" [] "rgb tex2" [1 1 1]',
                  'Material "metal" "texture eta" [] "rgb k" [1 1 1]', 'Material "metal" "rgb eta" [1 1 1] "rgb k" [1 1 1] "texture uroughness" [] "texture vroughness" "f"',
                  'Material "plastic" "texture roughness" []', 'LightSource "point" "texture I" []', 'AreaLightSource "diffuse" "texture L" []'):
        yield one("%s: a texture parameter with no value" % where, WORLD % (tex + where + '\nShape "sphere"'), must_refuse=True)
    for v, refuse in (("1e300", True), ("-1e300", True), ("-nan", True), ("+nan", True), ("+inf", True), ("-inf", True), ("2147483648", True), ("nan", True), ("inf", True), ("true", True), ("-1", False), ("0", False)):
        yield one("integer xresolution [%s]" % v, 'Film "image" "integer xresolution" [%s]\n' % v + WORLD % 'Shape "sphere"', must_refuse=refuse)
        yield one("integer pixelsamples %s" % v, 'Sampler "random" "integer pixelsamples" %s\n' % v + WORLD % 'Shape "sphere"', must_refuse=refuse)
        yield one("integer indices [0 1 %s]" % v, WORLD % TRI.replace("[0 1 2]", "[0 1 %s]" % v), must_refuse=refuse or v == "-1")
    for v in ("-1", "1000", "11", "1e300", "-nan", "-inf", "2147483648"):      # refused before anything is refined (a level count that is taken would refine on the GPU where there is one)
        yield one("loopsubdiv levels %s" % v, WORLD % (TETRA % v), must_refuse=True)
    yield one("Include of itself", features.replace('Include "inc.pbrt"', 'Include "s.pbrt"'), must_refuse=True)
    yield case("Include cycle through two files", dict(seed, **{"inc.pbrt": b'Include "b.pbrt"\n', "b.pbrt": b'Shape "sphere"\nInclude "inc.pbrt"\n'}), must_refuse=True)
    chain = {"inc.pbrt": b'Include "d0.pbrt"\n'}
    chain.update({"d%d.pbrt" % k: ('Include "d%d.pbrt"\n' % (k + 1)).encode() for k in range(40)})
    chain["d40.pbrt"] = b'Shape "sphere"\n'
    yield case("Include nested 42 deep", dict(seed, **chain), must_refuse=True)
    yield one("Include of a missing file", features.replace('Include "inc.pbrt"', 'Include "missing.pbrt"'), must_refuse=True)
    yield one("Include without a file name", WORLD % 'Include', must_refuse=True)
    yield one("Include inside a comment", features.replace('Include "inc.pbrt"', '# Include "missing.pbrt"\nInclude "inc.pbrt"  # Include "s.pbrt"'), same_as_seed=[])
    yield one("Include inside a string", features.replace('Film "image"', 'Film "image" "string filename" "Include.exr"'), same_as_seed=["film_name"])
    yield case("Include at two places of one file", dict(seed, **{"inc.pbrt": seed["inc.pbrt"] + b'Include "b.pbrt"\nInclude "b.pbrt"\n', "b.pbrt": b'Shape "sphere"\n'}))
    # the cases of the issue's table, by their names there
    yield one('Material "matte" before WorldBegin', 'Material "matte"\nCamera "perspective"\nWorldBegin\nWorldEnd\n', must_refuse=True)
    yield one("AttributeBegin before WorldBegin", 'AttributeBegin\nCamera "perspective"\nWorldBegin\nWorldEnd\n', must_refuse=True)
    sky = [a for a in exr_attrs(2, 2, 0)]
    sky[2][2] = struct.pack("<4i", 0, 0, 0x7ffffffe, 0x7ffffffe)
    yield case("infinite light whose .exr has dataWindow 0..0x7ffffffe", dict(seed, **{"s.pbrt": (WORLD % 'LightSource "infinite" "string mapname" "sky.exr"').encode(),
               "sky.exr": exr_assemble(sky, exr_blocks(exr_image(2, 2), 0))}), must_refuse=True)
    yield case("imagemap texture of a truncated .exr", dict(seed, **{"s.pbrt": (WORLD % 'Texture "i" "spectrum" "imagemap" "string filename" "t.exr"').encode(),
               "t.exr": exr_file(exr_image(4, 3), 0)[:-5]}), must_refuse=True)
    for what, ply in (("cut 5 bytes into its last face", seed["cube.ply"][:-8]), ("with element vertex 99999999999999", ply_file(normals=True, nv=99999999999999)[0])):
        yield case("plymesh " + what, dict(seed, **{"cube.ply": ply}), must_refuse=True)
    # non-finite and huge values delivered by a well-formed file: the loader may take them, and then the host BVH build must return
    for v in ("-nan", "+inf", "-inf", "3e38", "-3e38", "1e300"):
        yield one("P holds %s" % v, WORLD % TRI.replace("[0 0 0 1", "[0 0 %s 1" % v), nonfinite=True)
        yield one("N holds %s" % v, WORLD % (TRI + ' "normal N" [0 0 1 0 %s 1 0 0 1]' % v), nonfinite=True)
        yield one("uv holds %s" % v, WORLD % (TRI + ' "float uv" [0 0 1 %s 0 1]' % v), nonfinite=True)
        yield one("radius is %s" % v, WORLD % ('Shape "sphere" "float radius" %s\n' % v + TRI), nonfinite=True)
        yield one("Translate by %s" % v, WORLD % ('Translate 0 %s 0\nShape "sphere"\n' % v + TRI), nonfinite=True)
        yield one("Scale by %s" % v, WORLD % ('Scale 1 %s 1\nShape "sphere"\n' % v + TRI), nonfinite=True)
        # a mesh large enough for the BVH build to partition: 6 x 6 quads, every fifth vertex with one non-finite coordinate
        for every in (5, 2, 1):
            yield one("grid of 72 triangles, every %d. vertex holds %s" % (every, v), WORLD % grid_mesh(6, v, every), nonfinite=True)
        yield one("40 spheres, every third translated by %s" % v, WORLD % "\n".join(
            'AttributeBegin\nTranslate %s %d 0\nShape "sphere" "float radius" 0.25\nAttributeEnd' % (v if k % 3 == 0 else k, k % 7) for k in range(40)), nonfinite=True)
    for p, v, c in random_byte_cases(seed["s.pbrt"], rng_seed):
        c["data"] = dict(seed, **{"s.pbrt": c["data"]})
        yield c


# ------------------------------------------------------------------ families
def family_names():
    return ["exr-%s-%dx%d" % (v, w, h) for v in EXR_VARIANTS for (w, h) in EXR_SIZES] + [n for n, kw in ply_families()] + ["pbrt"]


def family(name, lib_write_exr=None):
    """-> (reader, seed, cases).  lib_write_exr(img) -> bytes is the library's own writer (needed by the exr-float families alone)."""
    k = family_names().index(name)
    if name.startswith("exr-"):
        _, variant, size = name.split("-")
        w, h = (int(x) for x in size.split("x"))
        seed = exr_seed(variant, w, h, lib_write_exr)
        return "exr", seed, exr_cases(seed, 1000 + k)
    if name == "pbrt":
        return "pbrt", pbrt_seed(), pbrt_cases(1000 + k)
    kw = dict(ply_families())[name]
    return "ply", ply_file(**kw)[0], ply_cases(kw, 1000 + k)


def free_share(name, seed):
    """The share of a seed's bytes that the format itself leaves free: a single-byte change there gives a file as valid as the seed, so no
    reader can refuse it.  EXR: the bytes of blocks stored raw, the literal bytes of RLE blocks (deflate blocks carry a checksum: none), and
    the values of displayWindow, pixelAspectRatio, screenWindowCenter and screenWindowWidth, which say nothing about the pixels.  Binary PLY:
    the vertex floats; every PLY: the text of the comment line.  Scene text: comments, and the names of parameters, which the format lets a
    file invent (a name nobody asks for is ignored, as in the reference).  A changed character of an ASCII number is almost never a digit."""
    import re
    if name.startswith("exr-"):
        attrs, offs, blocks, lay = exr_parse(seed)
        a = {x[0]: x[2] for x in attrs}
        x0, y0, x1, y1 = struct.unpack("<4i", a["dataWindow"])
        comp = a["compression"][0]
        row = sum((x1 - x0 + 1) * (4 if t == 2 else 2) for t in struct.unpack_from("<i", a["channels"], 2)[:1] * 3)
        free = 32
        for y, data in blocks:
            lines = min(16 if comp == 3 else 1, y1 - y + 1)
            if len(data) == row * lines:
                free += len(data)
            elif comp == 1:
                p = 0
                while p < len(data):
                    c = struct.unpack_from("b", data, p)[0]; p += 1
                    if c < 0:
                        free += -c; p += -c
                    else:
                        p += 1
        return free / len(seed)
    if name == "pbrt":
        text = seed["s.pbrt"].decode()
        free = sum(len(m.group(0)) - 1 for m in re.finditer(r"#[^\n]*", text)) + sum(len(m.group(1)) for m in re.finditer(r'"[a-z0-9]+ +([A-Za-z0-9]+)"', text))
        return free / len(text)
    kw = dict(ply_families())[name]
    free = len("made by tests/_corrupt_files.py") + (4 * (8 if kw["normals"] else 3) * len(PLY_P) if kw["binary"] else 0)
    return free / len(seed)


# ------------------------------------------------------------------ the walker (one child process per family)
def load_library(path):
    lib = C.CDLL(path)
    lib.ftn_exr_read.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ftn_exr_write.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32]
    lib.ftn_ply_load.argtypes = [C.c_char_p] + [C.c_void_p] * 8
    lib.ftn_pbrt_load.argtypes = [C.c_char_p, C.c_void_p]
    lib.ftn_pbrt_destroy.argtypes = [C.c_void_p]
    lib.ftn_pbrt_scene.argtypes = [C.c_void_p]; lib.ftn_pbrt_scene.restype = C.c_void_p
    lib.ftn_bvh_build.argtypes = [C.c_void_p] * 5
    for f in ("ftn_imageio_last_error", "ftn_pbrt_last_error"):
        getattr(lib, f).restype = C.c_char_p
    return lib


def writer_of(lib, scratch):
    def write(img):
        path = os.path.join(scratch, "seed_from_writer.exr")
        img = np.ascontiguousarray(img, np.float32)
        assert lib.ftn_exr_write(path.encode(), img.ctypes.data, img.shape[1], img.shape[0]) == 0
        with open(path, "rb") as f:
            return f.read()
    return write


def read_exr(lib, path):
    """-> (rc of the call that ended it, message, (w, h, words) or None)"""
    w, h = C.c_uint32(0xdeadbeef), C.c_uint32(0xdeadbeef)
    rc = lib.ftn_exr_read(path, C.byref(w), C.byref(h), None)
    if rc:
        return rc, lib.ftn_imageio_last_error(), None
    if w.value * h.value * 12 > os.path.getsize(path) * 2048 + (1 << 20):
        return rc, b"", (w.value, h.value, None)                  # no file of this size packs that many pixels: reported by check_exr, not allocated
    px = np.full(w.value * h.value * 3, SENTINEL, np.uint32)
    w2, h2 = C.c_uint32(0), C.c_uint32(0)
    rc = lib.ftn_exr_read(path, C.byref(w2), C.byref(h2), px.ctypes.data)
    if rc:
        return rc, lib.ftn_imageio_last_error(), None
    return rc, b"", ((w.value, h.value) if (w2.value, h2.value) == (w.value, h.value) else (w.value, h.value, w2.value, h2.value)) + (px,)


def read_ply(lib, path):
    nv, nt, hn, hu = C.c_uint32(0xdeadbeef), C.c_uint32(0xdeadbeef), C.c_int(-7), C.c_int(-7)
    rc = lib.ftn_ply_load(path, C.byref(nv), C.byref(nt), None, None, None, None, C.byref(hn), C.byref(hu))
    if rc:
        return rc, lib.ftn_pbrt_last_error(), None
    if (nv.value + nt.value) * 4 > os.path.getsize(path) + 64:
        return rc, b"", (nv.value, nt.value, None)
    P, N, UV = (np.full(nv.value * k, SENTINEL, np.uint32) for k in (3, 3, 2))
    F = np.full(nt.value * 3, 0xffffffff, np.uint32)
    nv2, nt2 = C.c_uint32(0), C.c_uint32(0)
    rc = lib.ftn_ply_load(path, C.byref(nv2), C.byref(nt2), P.ctypes.data, N.ctypes.data, UV.ctypes.data, F.ctypes.data, C.byref(hn), C.byref(hu))
    if rc:
        return rc, lib.ftn_pbrt_last_error(), None
    return rc, b"", (nv.value, nt.value, dict(P=P, N=N if hn.value else None, UV=UV if hu.value else None, F=F, again=(nv2.value, nt2.value), flags=(hn.value, hu.value)))


def read_pbrt(lib, path, be):
    from fountain_amd import FountainError, PbrtScene
    from test_reader_descriptors import descriptor_hashes
    try:
        ps = PbrtScene(path.decode(), be)
    except FountainError as e:
        return e.code, be.lib.ftn_pbrt_last_error(), None
    n = C.c_uint32()
    return 0, b"", dict(hashes=descriptor_hashes(ps), bvh=lib.ftn_bvh_build(C.addressof(ps.desc), None, None, C.addressof(n), None))


def check_common(c, rc, msg):
    out = []
    if rc not in ALLOWED:
        out.append("returned %d, which is none of FTN_OK, INVALID_ARGUMENT, UNSUPPORTED, OUT_OF_MEMORY" % rc)
    if rc != 0 and not msg:
        out.append("refused with %d and no message" % rc)
    if rc == 0 and c["must_refuse"]:
        out.append("accepted (FTN_OK), must be refused")
    return out


def check_exr(c, rc, msg, got, seed_px):
    out = check_common(c, rc, msg)
    if rc == 0:
        if len(got) != 3:
            return out + ["the sizing call said %d x %d, the filling call %d x %d" % got[:4]]
        w, h, px = got
        if px is None:
            return out + ["the sizing call reports %d x %d pixels for a file of %d bytes" % (w, h, len(c["data"]))]
        if exr_window(c["data"]) != (w, h):
            out.append("size %d x %d is not the data window %r" % (w, h, exr_window(c["data"])))
        left = int((px == SENTINEL).sum())
        if left:
            out.append("accepted, but %d of %d output words were never written" % (left, px.size))
        if c.get("same_pixels") and not np.array_equal(px, seed_px):
            out.append("accepted, but the pixels are not the seed's")
    return out


def check_ply(c, rc, msg, got, seed_mesh):
    out = check_common(c, rc, msg)
    if rc == 0:
        nv, nt, m = got
        if m is None:
            return out + ["the sizing call reports %d vertices and %d triangles for a file of %d bytes" % (nv, nt, len(c["data"]))]
        if m["again"] != (nv, nt):
            out.append("the sizing call said %d / %d, the filling call %d / %d" % ((nv, nt) + m["again"]))
        for k in ("P", "N", "UV"):
            if m[k] is not None and (m[k] == SENTINEL).any():
                out.append("accepted, but %d words of %s were never written" % (int((m[k] == SENTINEL).sum()), k))
        if (m["F"] >= nv).any():
            out.append("accepted with vertex index %d of %d vertices" % (int(m["F"].max()), nv))
        if c.get("counts") is not None and (nv, nt) != tuple(c["counts"]):
            out.append("accepted with %d vertices and %d triangles, the file has %d and %d" % ((nv, nt) + tuple(c["counts"])))
        F, F0 = m["F"].reshape(-1, 3), seed_mesh["F"].reshape(-1, 3)
        for t in c.get("tris") or []:
            if t >= len(F) or not np.array_equal(F[t], F0[t]):
                out.append("triangle %d is %s, the file says %s" % (t, "missing" if t >= len(F) else tuple(int(x) for x in F[t]), tuple(int(x) for x in F0[t])))
                break
    return out


def check_pbrt(c, rc, msg, got, seed_hashes):
    out = check_common(c, rc, msg)
    if c.get("same_as_seed") is not None:
        if rc != 0:
            out.append("refused (%d: %s): the word Include in a comment or a string is not a statement" % (rc, msg.decode(errors="replace")))
        else:
            diff = sorted(k for k in seed_hashes if got["hashes"][k] != seed_hashes[k])
            if diff != sorted(c["same_as_seed"]):
                out.append("descriptors differ from the seed's in %r, expected %r" % (diff, c["same_as_seed"]))
    return out


def walk(name, lib_path, scratch, progress_path, report_path, start=0):
    sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
    lib = load_library(lib_path)
    reader, seed, cases = family(name, writer_of(lib, scratch))
    report = dict(done=False, n_cases=0, n_random=0, n_random_ok=0, failures=[])

    def save():
        with open(report_path + ".tmp", "w") as f:
            json.dump(report, f)
        os.replace(report_path + ".tmp", report_path)

    def note(case_name, what):
        if len(report["failures"]) < 200:
            report["failures"].append([case_name, what])
            save()                                       # what was found survives a crash further on

    def put(dirpath, files):
        os.makedirs(dirpath, exist_ok=True)
        for fn, data in files.items():
            with open(os.path.join(dirpath, fn), "wb") as f:
                f.write(data)

    seed_dir, case_dir = os.path.join(scratch, "seed"), os.path.join(scratch, "case")
    main = {"exr": "a.exr", "ply": "a.ply", "pbrt": "s.pbrt"}[reader]
    put(seed_dir, seed if reader == "pbrt" else {main: seed})
    seed_path, case_path = os.path.join(seed_dir, main).encode(), os.path.join(case_dir, main).encode()
    if reader == "pbrt":
        from fountain_amd.api import Backend
        be = Backend(lib_path)
        read = lambda p: read_pbrt(lib, p, be)
        bits = lambda got: got["hashes"]
    elif reader == "exr":
        read, bits = (lambda p: read_exr(lib, p)), (lambda got: got[-1].tobytes() if len(got) == 3 and got[2] is not None else None)
    else:
        read = lambda p: read_ply(lib, p)
        bits = lambda got: None if got[2] is None else [None if got[2][k] is None else got[2][k].tobytes() for k in ("P", "N", "UV", "F")]
    prog = os.open(progress_path, os.O_WRONLY | os.O_CREAT | os.O_APPEND)
    os.write(prog, b"(the untouched seed)\n")
    rc, msg, got = read(seed_path)
    if rc != 0:
        note("(the untouched seed)", "refused: %d %s" % (rc, msg.decode(errors="replace")))
    seed_bits = bits(got) if rc == 0 else None
    seed_ref = None if rc != 0 else got[2] if reader != "pbrt" else got["hashes"]
    for k, c in enumerate(cases):
        if k < start:
            continue
        os.write(prog, (c["name"] + "\n").encode())
        if reader == "pbrt":
            for fn in os.listdir(case_dir) if os.path.isdir(case_dir) else []:
                os.remove(os.path.join(case_dir, fn))
        put(case_dir, c["data"] if reader == "pbrt" else {main: c["data"]})
        rc, msg, got = read(case_path)
        check = {"exr": check_exr, "ply": check_ply, "pbrt": check_pbrt}[reader]
        for what in check(c, rc, msg, got, seed_ref):
            note(c["name"], what)
        report["n_cases"] += 1
        if c["random"]:
            report["n_random"] += 1
            report["n_random_ok"] += rc == 0
        if rc != 0 and seed_bits is not None:                     # no state is left behind: the seed still gives the seed's bits
            rc2, msg2, got2 = read(seed_path)
            if rc2 != 0 or bits(got2) != seed_bits:
                note(c["name"], "after this refusal the untouched seed %s" % ("is refused: %d" % rc2 if rc2 else "reads back with other bits"))
    os.write(prog, b"(done)\n")
    report["done"] = True
    save()


# ------------------------------------------------------------------ the corpus on disk, for tools/reader_check.cpp
def write_corpus(dirpath, lib_path, n_random=N_RANDOM):
    """DIR/<family>/<k>[.ext or /s.pbrt] and DIR/manifest.txt: one line `reader<TAB>must_refuse<TAB>relative path<TAB>name` a case."""
    sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
    lib = load_library(lib_path)
    os.makedirs(dirpath, exist_ok=True)
    lines = []
    for name in family_names():
        reader, seed, cases = family(name, writer_of(lib, dirpath))
        os.makedirs(os.path.join(dirpath, name), exist_ok=True)
        n_rand = 0
        for k, c in enumerate([case("(the untouched seed)", seed)] + list(cases)):
            if c["random"]:
                n_rand += 1
                if n_rand > n_random:
                    continue
            if reader == "pbrt":
                rel = "%s/%d/s.pbrt" % (name, k)
                os.makedirs(os.path.join(dirpath, name, str(k)), exist_ok=True)
                for fn, data in c["data"].items():
                    with open(os.path.join(dirpath, name, str(k), fn), "wb") as f:
                        f.write(data)
            else:
                rel = "%s/%d.%s" % (name, k, reader)
                with open(os.path.join(dirpath, rel), "wb") as f:
                    f.write(c["data"])
            lines.append("%s\t%d\t%s\t%s\n" % (reader, c["must_refuse"], rel, c["name"].replace("\t", " ").replace("\n", " ")))
    with open(os.path.join(dirpath, "manifest.txt"), "w") as f:
        f.writelines(lines)
    return len(lines)


def default_library():
    return os.path.join(os.path.dirname(HERE), "fountain_amd", os.environ.get("FTN_LIB", "libfountain_hip.so"))


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", metavar="DIR", help="write every case and manifest.txt into DIR")
    ap.add_argument("--random", type=int, default=N_RANDOM, help="random cases per seed written by --write")
    ap.add_argument("--walk", metavar="FAMILY", help="walk one family's cases (the child process of test_corrupt_files.py)")
    ap.add_argument("--lib", default=default_library())
    ap.add_argument("--scratch"); ap.add_argument("--progress"); ap.add_argument("--report"); ap.add_argument("--start", type=int, default=0)
    ap.add_argument("--list", action="store_true", help="print the family names")
    o = ap.parse_args()
    if o.list:
        print("\n".join(family_names()))
    if o.write:
        print("%d cases written to %s" % (write_corpus(o.write, o.lib, o.random), o.write))
    if o.walk:
        walk(o.walk, o.lib, o.scratch, o.progress, o.report, o.start)
