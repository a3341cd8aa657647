"""An independent numpy restatement of the display stage (include/fountain_hip_display.h), sharing no code with the library: the
luminance histogram in float32 and integers, the exposure in float64, the encode in float64 (the library's is binary32), the Bayer
matrix written out again, and a PNG reader from the PNG specification with struct and zlib."""
import struct
import zlib

import numpy as np

F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)
HIST_WORDS, BINS, INVALID, BELOW, ABOVE = 388, 384, 384, 385, 386
TONEMAPS = ("linear", "reinhard", "aces", "hable")
TRANSFERS = ("srgb", "gamma", "linear")

BAYER = np.array([[0, 32, 8, 40, 2, 34, 10, 42],
                  [48, 16, 56, 24, 50, 18, 58, 26],
                  [12, 44, 4, 36, 14, 46, 6, 38],
                  [60, 28, 52, 20, 62, 30, 54, 22],
                  [3, 35, 11, 43, 1, 33, 9, 41],
                  [51, 19, 59, 27, 49, 17, 57, 25],
                  [15, 47, 7, 39, 13, 45, 5, 37],
                  [63, 31, 55, 23, 61, 29, 53, 21]], np.int64)


def log_uniform(rng, shape, lo=-12.0, hi=6.0):
    """float32 values whose log2 is uniform in [lo, hi]"""
    return np.exp2(rng.uniform(lo, hi, shape)).astype(F32)


def luminance32(rgb):
    rgb = np.asarray(rgb, F32)
    with np.errstate(all="ignore"):
        return (rgb[..., 0] * F32(0.212671) + rgb[..., 1] * F32(0.715160)) + rgb[..., 2] * F32(0.072169)


def histogram(rgb):
    """the header's 388 words from the luminance's bits"""
    Y = luminance32(rgb).ravel()
    hist = np.zeros(HIST_WORDS, np.uint32)
    with np.errstate(invalid="ignore"):
        ok = Y >= 0
        below = ok & (Y < F32(2.0 ** -24))
        above = ok & (Y >= F32(2.0 ** 24))
    inside = ok & ~below & ~above
    hist[INVALID], hist[BELOW], hist[ABOVE] = (~ok).sum(), below.sum(), above.sum()
    base = int(np.array([2.0 ** -24], F32).view(np.uint32)[0] >> 20)
    bins = (Y[inside].view(np.uint32) >> 20).astype(np.int64) - base
    assert bins.size == 0 or (bins.min() >= 0 and bins.max() < BINS)
    hist[:BINS] = np.bincount(bins, minlength=BINS)
    return hist


def bin_of(Y):
    """the bin of one luminance inside [2^-24, 2^24), from its logarithm (not its bits): eight per octave, linear within the octave"""
    o = int(np.floor(np.log2(float(Y))))
    m = int(np.floor((float(Y) / 2.0 ** o - 1.0) * 8.0))
    return 8 * (o + 24) + m


def bin_representative(i):
    return (i // 8 - 24) + np.log2(1.0 + ((i % 8) + 0.5) / 8.0)


def exposure64(hist, auto=True, ev=0.0, key=0.18, p_lo=0.10, p_hi=0.95, min_ev=-16.0, max_ev=16.0):
    """(scale as float64 before the rounding to binary32, avg_log2, empty)"""
    if not auto:
        return 2.0 ** float(ev), 0.0, False
    n = np.asarray(hist[:BINS], np.float64)
    t = n.sum()
    if t == 0:
        return 1.0, 0.0, True
    lo, hi = float(F32(p_lo)) * t, float(F32(p_hi)) * t
    c = np.concatenate([[0.0], np.cumsum(n)])
    wgt = np.maximum(0.0, np.minimum(c[1:], hi) - np.maximum(c[:-1], lo))
    rep = np.array([bin_representative(i) for i in range(BINS)])
    avg = float((wgt * rep).sum() / wgt.sum())
    s = float(F32(key)) / 2.0 ** avg
    return min(max(s, 2.0 ** float(min_ev)), 2.0 ** float(max_ev)), avg, False


def _clamp01(v):
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, np.minimum(v, 1.0), 0.0)


def _hable(x):
    A, B, C, D, E, F = 0.15, 0.50, 0.10, 0.20, 0.02, 0.30
    return (x * (A * x + C * B) + D * E) / (x * (A * x + B) + D * F) - E / F


def display64(rgb, scale=1.0, tonemap="aces", transfer="srgb", white=11.2, gamma=2.2):
    """steps 1 to 3 in float64 with the decimal constants: the display-referred image [H, W, 3]"""
    with np.errstate(invalid="ignore"):
        c = np.asarray(rgb, F32).astype(np.float64) * float(F32(scale))
        c = np.where(c > 0, np.minimum(c, 65504.0), 0.0)
    white = float(F32(white))
    if tonemap == "reinhard":
        L = c[..., 0] * 0.212671 + c[..., 1] * 0.715160 + c[..., 2] * 0.072169
        with np.errstate(all="ignore"):
            s = np.where(L == 0, 1.0, (L * (1.0 + L / (white * white))) / (1.0 + L) / np.where(L == 0, 1.0, L))
        c = c * s[..., None]
    elif tonemap == "aces":
        c = (c * (2.51 * c + 0.03)) / (c * (2.43 * c + 0.59) + 0.14)
    elif tonemap == "hable":
        c = _hable(c) / _hable(white)
    else:
        assert tonemap == "linear"
    v = _clamp01(c)
    if transfer == "srgb":
        v = np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(v, 1.0 / 2.4) - 0.055)
    elif transfer == "gamma":
        v = np.power(v, 1.0 / float(F32(gamma)))
    else:
        assert transfer == "linear"
    return _clamp01(v)


def dither_offsets(h, w):
    """d of every pixel, [H, W]"""
    y, x = np.mgrid[0:h, 0:w]
    return (BAYER[y & 7, x & 7] + 0.5) / 64.0 - 0.5


def quantise64(v, dither=False):
    """(codes [H, W, 3] as int64, the value v * 255 + 0.5 + d before the floor)"""
    q = v * 255.0 + 0.5
    if dither:
        q = q + dither_offsets(*v.shape[:2])[..., None]
    return np.clip(np.floor(q), 0, 255).astype(np.int64), q


def unpack(rgba8):
    """uint32 [H, W] -> (codes [H, W, 3] as int64, alpha [H, W])"""
    a = np.asarray(rgba8, np.uint32)
    return np.stack([(a >> s) & 0xff for s in (0, 8, 16)], axis=-1).astype(np.int64), (a >> 24).astype(np.int64)


# ------------------------------------------------------------------ PNG, from the specification (ISO/IEC 15948, sections 5 and 11)
PNG_SIGNATURE = bytes([137, 80, 78, 71, 13, 10, 26, 10])


def read_png(path):
    """Every chunk's CRC is checked.  Returns a dict: chunks (the type names in file order), width, height, bit_depth, colour_type,
    compression, filter_method, interlace, srgb_intent / gama (None when the chunk is absent), filters (the filter byte of every
    scanline) and pixels (uint8 [H, W, 3]; only 8-bit RGB without interlace is decoded, every filter type undone)."""
    data = open(path, "rb").read()
    assert data[:8] == PNG_SIGNATURE, "not a PNG signature"
    p, chunks, idat, out = 8, [], b"", dict(srgb_intent=None, gama=None)
    while p < len(data):
        n, kind = struct.unpack(">I4s", data[p:p + 8])
        body = data[p + 8:p + 8 + n]
        crc, = struct.unpack(">I", data[p + 8 + n:p + 12 + n])
        assert len(body) == n and zlib.crc32(kind + body) & 0xffffffff == crc, "bad CRC in %r" % kind
        chunks.append(kind.decode("ascii"))
        if kind == b"IHDR":
            assert n == 13
            out["width"], out["height"], out["bit_depth"], out["colour_type"], out["compression"], out["filter_method"], out["interlace"] = \
                struct.unpack(">IIBBBBB", body)
        elif kind == b"sRGB":
            assert n == 1
            out["srgb_intent"] = body[0]
        elif kind == b"gAMA":
            assert n == 4
            out["gama"], = struct.unpack(">I", body)
        elif kind == b"IDAT":
            idat += body
        p += 12 + n
    assert p == len(data) and chunks[-1] == "IEND"
    out["chunks"] = chunks
    assert (out["bit_depth"], out["colour_type"], out["interlace"]) == (8, 2, 0), "only 8-bit RGB without interlace is decoded"
    w, h = out["width"], out["height"]
    raw = zlib.decompress(idat)
    stride = 1 + 3 * w
    assert len(raw) == stride * h
    rows = np.frombuffer(raw, np.uint8).reshape(h, stride)
    out["filters"] = rows[:, 0].copy()
    px = np.zeros((h, 3 * w), np.int64)
    for y in range(h):
        f, line = int(rows[y, 0]), rows[y, 1:].astype(np.int64)
        up = px[y - 1] if y else np.zeros(3 * w, np.int64)
        if f in (0, 2):
            px[y] = (line + (up if f == 2 else 0)) & 0xff
            continue
        for i in range(3 * w):
            a = px[y, i - 3] if i >= 3 else 0
            b, c = up[i], (up[i - 3] if i >= 3 else 0)
            if f == 1:
                pred = a
            elif f == 3:
                pred = (a + b) // 2
            else:
                assert f == 4
                pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            px[y, i] = (line[i] + pred) & 0xff
    out["pixels"] = px.astype(np.uint8).reshape(h, w, 3)
    return out


def pixel_with_luminance(target, rng=None):
    """An rgb pixel (float32 [3]) whose binary32 luminance, in the header's operation order, is exactly `target` (> 0, finite): green
    alone where a green value exists, else a random share of red with the green searched a few ulps around the quotient."""
    rng = rng or np.random.default_rng(7)
    target = F32(target)
    for attempt in range(4096):
        r = F32(0.0) if attempt == 0 else F32(rng.uniform(0.0, 0.9) * float(target) / 0.212671)
        g = F32((float(target) - float(r) * 0.212671) / 0.715160)
        cand = [g]
        for _ in range(6):
            cand = [np.nextafter(cand[0], F32(0.0))] + cand + [np.nextafter(cand[-1], F32(np.inf))]
        px = np.zeros((len(cand), 3), F32)
        px[:, 0], px[:, 1] = r, np.array(cand, F32)
        hit = np.nonzero(luminance32(px) == target)[0]
        if hit.size:
            return px[hit[0]]
    raise AssertionError("no pixel found whose luminance is %r" % target)


# ------------------------------------------------------------------ the test images, shared by the CPU and the GPU tests
def images():
    """name -> rgb [H, W, 3] float32; made once (the GPU tests use them too)"""
    rng = np.random.default_rng(20240607)
    out = {}
    for h, w in ((1, 1), (3, 1), (1, 3), (7, 5), (53, 37), (255, 257)):
        out["random %dx%d" % (w, h)] = log_uniform(rng, (h, w, 3), -30.0, 30.0)
    out["constant 512x512"] = np.full((512, 512, 3), 0.35, F32)
    checker = np.zeros((64, 48, 3), F32)
    yy, xx = np.mgrid[0:64, 0:48]
    checker[...] = np.where(((yy + xx) & 1)[..., None] == 0, F32(0.02), F32(3.0))
    out["checker 48x64"] = checker
    out["salted 37x53"] = salted(rng)
    return out


SALT = [("nan", NAN, INVALID), ("+inf", INF, ABOVE), ("-inf", -INF, INVALID), ("-1", F32(-1.0), INVALID), ("0", F32(0.0), BELOW),
        ("-0", F32(-0.0), BELOW), ("subnormal", F32(1e-40), BELOW), ("2^-24", F32(2.0 ** -24), 0),
        ("below 2^-24", np.nextafter(F32(2.0 ** -24), F32(0.0)), BELOW), ("2^24", F32(2.0 ** 24), ABOVE),
        ("below 2^24", np.nextafter(F32(2.0 ** 24), F32(0.0)), BINS - 1)]


def salt_pixel(value):
    """a pixel whose luminance is exactly `value` (for -1: some negative finite luminance)"""
    if not np.isfinite(value) or value <= 0:
        return np.array([0.0, value, 0.0], F32)                     # 0 * a + v * b + 0 * c: NaN, the infinities, -1 and the zeros survive
    return pixel_with_luminance(value)


def salted(rng):
    img = log_uniform(rng, (53, 37, 3))
    for k, (_, value, _) in enumerate(SALT):
        img[3 + 4 * k, 5 + 2 * k] = salt_pixel(value)
    return img
