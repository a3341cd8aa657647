/*
 * ftn_imageio.cpp -- the output stage's file format: OpenEXR scanline images with 32-bit float R, G, B channels, as
 * write_exr / read_exr produce and consume (src/imageio/exr.rs:11-87).  The reference delegates the container to the `exr`
 * crate (RLE-compressed scanline blocks); this writer emits the same layer (name "image", channels B G R, FLOAT, increasing
 * line order) with NO_COMPRESSION, which every OpenEXR reader accepts and which keeps the sample bits exactly as rendered.
 * The reader handles NO_COMPRESSION, RLE, ZIPS and ZIP scanline files with FLOAT or HALF channels (what the writer above and the
 * reference's writer produce, plus the usual encoding of environment maps and textures found in PBRT scenes; zlib inflates).
 */
#include "../../include/fountain_hip.h"
#include "../../include/fountain_hip_idmatte.h"
#include "detmath.h"

#include <algorithm>
#include <cstdio>
#include <zlib.h>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

namespace {

thread_local std::string g_io_err;
int io_fail(int code, const std::string& m) { g_io_err = m; return code; }

void put_i32(std::vector<unsigned char>& b, int32_t v) { unsigned char t[4]; memcpy(t, &v, 4); b.insert(b.end(), t, t + 4); }
void put_f32(std::vector<unsigned char>& b, float v) { unsigned char t[4]; memcpy(t, &v, 4); b.insert(b.end(), t, t + 4); }
void put_str(std::vector<unsigned char>& b, const char* s) { b.insert(b.end(), s, s + strlen(s) + 1); }
void put_attr(std::vector<unsigned char>& b, const char* name, const char* type, const std::vector<unsigned char>& data) {
    put_str(b, name); put_str(b, type); put_i32(b, (int32_t)data.size()); b.insert(b.end(), data.begin(), data.end());
}

float half_to_float(uint16_t h) {
    const uint32_t s = (uint32_t)(h >> 15) << 31, e = (h >> 10) & 31u, m = h & 1023u;
    uint32_t u;
    if (e == 0) {
        if (m == 0) u = s;
        else { int sh = 0; uint32_t mm = m; while (!(mm & 1024u)) { mm <<= 1; sh++; } u = s | ((uint32_t)(113 - sh) << 23) | ((mm & 1023u) << 13); }
    } else if (e == 31) u = s | 0x7f800000u | (m << 13);
    else u = s | ((e + 112u) << 23) | (m << 13);
    float f; memcpy(&f, &u, 4); return f;
}

/* the byte predictor and the two-halves interleave shared by OpenEXR's RLE and ZIP blocks */
void unpredict(std::vector<unsigned char>& tmp, std::vector<unsigned char>& out) {
    const size_t n = tmp.size();
    for (size_t i = 1; i < n; i++) tmp[i] = (unsigned char)(tmp[i - 1] + tmp[i] - 128);
    out.resize(n);
    const size_t half = (n + 1) / 2;
    for (size_t i = 0, a = 0, b = half; i < n;) { out[i++] = tmp[a++]; if (i < n) out[i++] = tmp[b++]; }
}
/* OpenEXR RLE block: run-length bytes, then predictor + interleave undone */
bool rle_decode(const unsigned char* in, size_t n_in, std::vector<unsigned char>& out, size_t n_out) {
    std::vector<unsigned char> tmp; tmp.reserve(n_out);
    size_t p = 0;
    while (p < n_in) {
        const int c = (signed char)in[p++];
        if (c < 0) { const size_t k = (size_t)(-c); if (p + k > n_in) return false; tmp.insert(tmp.end(), in + p, in + p + k); p += k; }
        else { if (p >= n_in) return false; tmp.insert(tmp.end(), (size_t)c + 1, in[p]); p++; }
        if (tmp.size() > n_out) return false;
    }
    if (tmp.size() != n_out) return false;
    unpredict(tmp, out);
    return true;
}
bool zip_decode(const unsigned char* in, size_t n_in, std::vector<unsigned char>& out, size_t n_out) {
    std::vector<unsigned char> tmp(n_out);
    uLongf got = (uLongf)n_out;
    if (uncompress(tmp.data(), &got, in, (uLong)n_in) != Z_OK || got != n_out) return false;
    unpredict(tmp, out);
    return true;
}

/* nothing unwinds across the C boundary: a failed allocation (or a size no allocation can have) is FTN_ERR_OUT_OF_MEMORY, anything
 * else FTN_ERR_INTERNAL; the locals of the call, an open file among them, are released on the way */
template <class F> int guarded(F&& f) {
    try { return f(); }
    catch (const std::bad_alloc&) { return io_fail(FTN_ERR_OUT_OF_MEMORY, "out of memory"); }
    catch (const std::length_error&) { return io_fail(FTN_ERR_OUT_OF_MEMORY, "out of memory (a size no allocation can have)"); }
    catch (const std::exception& e) { return io_fail(FTN_ERR_INTERNAL, e.what()); }
}
struct File {
    FILE* f;
    explicit File(FILE* f_) : f(f_) {}
    ~File() { if (f) fclose(f); }
    int close() { FILE* g = f; f = nullptr; return g ? fclose(g) : 0; }
    File(const File&) = delete; File& operator=(const File&) = delete;
};

/* The one way the reader looks at a file's bytes: every read names the bytes it needs and fails when they are not there, so no
 * length, count or string found in the file can move a read past the end of what the file (or one attribute of it) holds. */
struct Cursor {
    const unsigned char* b; size_t n, p;
    size_t left() const { return n - p; }
    bool bytes(size_t k, const unsigned char** out) { if (k > left()) return false; *out = b + p; p += k; return true; }
    bool i32(int32_t* v) { const unsigned char* s; if (!bytes(4, &s)) return false; memcpy(v, s, 4); return true; }
    bool u64(uint64_t* v) { const unsigned char* s; if (!bytes(8, &s)) return false; memcpy(v, s, 8); return true; }
    bool cstr(std::string* s) {
        const unsigned char* e = left() ? (const unsigned char*)memchr(b + p, 0, left()) : nullptr;
        if (!e) return false;
        s->assign((const char*)(b + p), (size_t)(e - (b + p))); p = (size_t)(e - b) + 1; return true;
    }
};

/* The most pixels a file may declare (include/fountain_hip.h): 2^28, a 3 GiB RGB float image.  The data window of a corrupt file
 * is any pair of int32 corners; without a cap the caller of the sizing call is told to allocate up to 2^64 pixels. */
const uint64_t EXR_MAX_PIXELS = (uint64_t)1 << 28;
/* deflate cannot shrink below 1 : 1032 and OpenEXR's RLE not below 1 : 64: a block that claims more is corrupt, and is refused
 * before anything of the claimed size is allocated */
const uint64_t EXR_MAX_RATIO = 1040;

int exr_read(const char* path, uint32_t* w_out, uint32_t* h_out, float* rgb_out) {
    if (!path) return io_fail(FTN_ERR_INVALID_ARGUMENT, "ftn_exr_read: bad arguments");
    std::vector<unsigned char> buf;
    {
        File f(fopen(path, "rb"));
        if (!f.f) return io_fail(FTN_ERR_INVALID_ARGUMENT, std::string("cannot open ") + path);
        unsigned char tmp[65536]; size_t n; while ((n = fread(tmp, 1, sizeof(tmp), f.f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
    }
    if (buf.size() < 8 || buf[0] != 0x76 || buf[1] != 0x2f || buf[2] != 0x31 || buf[3] != 0x01) return io_fail(FTN_ERR_INVALID_ARGUMENT, std::string(path) + ": not an OpenEXR file");
    if (buf[5] & 0x1a) return io_fail(FTN_ERR_UNSUPPORTED, "tiled / deep / multi-part OpenEXR files are not supported");
    if (buf[4] != 2 || (buf[5] & ~0x04) || buf[6] || buf[7]) return io_fail(FTN_ERR_INVALID_ARGUMENT, "OpenEXR version field is not version 2 with known flags");
    Cursor c{buf.data(), buf.size(), 8};
    struct Chan { std::string name; int type; };
    std::vector<Chan> chans; int compression = -1; int32_t dw[4] = {0, 0, -1, -1};
    /* the attributes every OpenEXR header has, each of its type and size (the four that say nothing about the pixels are only looked at
     * that far): a file without one of them was not written as OpenEXR, or is no longer what was written */
    static const struct { const char* name; const char* type; int32_t size; } required[] = {
        {"channels", "chlist", -1}, {"compression", "compression", 1}, {"dataWindow", "box2i", 16}, {"displayWindow", "box2i", 16}, {"lineOrder", "lineOrder", 1},
        {"pixelAspectRatio", "float", 4}, {"screenWindowCenter", "v2f", 8}, {"screenWindowWidth", "float", 4}};
    unsigned have = 0;
    for (;;) {
        std::string name, type; int32_t size; const unsigned char* a;
        if (!c.cstr(&name)) return io_fail(FTN_ERR_INVALID_ARGUMENT, "truncated OpenEXR header");
        if (name.empty()) break;
        if (!c.cstr(&type) || !c.i32(&size) || size < 0 || !c.bytes((size_t)size, &a)) return io_fail(FTN_ERR_INVALID_ARGUMENT, "truncated OpenEXR header");
        Cursor at{a, (size_t)size, 0};                         /* an attribute is read through its own size, never past it */
        for (unsigned k = 0; k < 8; k++) if (name == required[k].name) {
            if (type != required[k].type || (required[k].size >= 0 && size != required[k].size) || (have & (1u << k)))
                return io_fail(FTN_ERR_INVALID_ARGUMENT, "OpenEXR attribute " + name + " has the wrong type or size, or is given twice");
            have |= 1u << k;
        }
        if (name == "channels") {
            for (;;) {
                Chan ch; int32_t t, sampling[2]; const unsigned char* lin;
                if (!at.cstr(&ch.name)) return io_fail(FTN_ERR_INVALID_ARGUMENT, "corrupt OpenEXR channel list");
                if (ch.name.empty()) break;
                if (!at.i32(&t) || !at.bytes(4, &lin) || !at.i32(&sampling[0]) || !at.i32(&sampling[1]) || lin[0] > 1 || lin[1] || lin[2] || lin[3])
                    return io_fail(FTN_ERR_INVALID_ARGUMENT, "corrupt OpenEXR channel list");
                if (sampling[0] != 1 || sampling[1] != 1) return io_fail(FTN_ERR_UNSUPPORTED, "subsampled OpenEXR channels are not supported");
                ch.type = t; chans.push_back(ch);
            }
            if (at.left()) return io_fail(FTN_ERR_INVALID_ARGUMENT, "corrupt OpenEXR channel list");
        } else if (name == "compression") compression = a[0];
        else if (name == "dataWindow") memcpy(dw, a, 16);
        else if (name == "lineOrder") { if (a[0] > 1) return io_fail(FTN_ERR_INVALID_ARGUMENT, "OpenEXR scanline files are stored in increasing or decreasing y"); }   /* every block carries its own y */
        else if (name == "displayWindow") { int32_t d[4]; memcpy(d, a, 16); if (d[2] < d[0] || d[3] < d[1]) return io_fail(FTN_ERR_INVALID_ARGUMENT, "OpenEXR displayWindow is empty"); }
    }
    for (unsigned k = 0; k < 8; k++) if (!(have & (1u << k))) return io_fail(FTN_ERR_INVALID_ARGUMENT, std::string("OpenEXR header has no ") + required[k].name + " attribute");
    const int64_t w = (int64_t)dw[2] - dw[0] + 1, h = (int64_t)dw[3] - dw[1] + 1;
    if (w <= 0 || h <= 0) return io_fail(FTN_ERR_INVALID_ARGUMENT, "OpenEXR file has no dataWindow");
    if (compression < 0 || compression > 3) return io_fail(FTN_ERR_UNSUPPORTED, "only NO_COMPRESSION, RLE, ZIPS and ZIP OpenEXR scanline files are supported (not PIZ / PXR24 / B44 / DWA)");
    if (w > (int64_t)0xffffffff || h > (int64_t)0xffffffff || (uint64_t)w > EXR_MAX_PIXELS / (uint64_t)h)
        return io_fail(FTN_ERR_INVALID_ARGUMENT, "OpenEXR dataWindow holds more than 2^28 pixels");
    const uint64_t lines_per_block = compression == 3 ? 16 : 1;
    int ci[3] = {-1, -1, -1}; uint64_t row_bytes = 0; std::vector<uint64_t> ch_off(chans.size());
    for (size_t k = 0; k < chans.size(); k++) {
        ch_off[k] = row_bytes;
        if (chans[k].type != 1 && chans[k].type != 2) return io_fail(FTN_ERR_UNSUPPORTED, "UINT OpenEXR channels are not supported");   /* read_exr panics */
        row_bytes += (uint64_t)w * (chans[k].type == 2 ? 4 : 2);            /* w <= 2^28 and a channel costs 18 bytes of file: no overflow */
        if (chans[k].name == "R") ci[0] = (int)k; else if (chans[k].name == "G") ci[1] = (int)k; else if (chans[k].name == "B") ci[2] = (int)k;
    }
    if (ci[0] < 0 || ci[1] < 0 || ci[2] < 0) return io_fail(FTN_ERR_INVALID_ARGUMENT, "OpenEXR file lacks R, G or B");
    /* the offset table and every block header are checked by the sizing call as well: a size it reports belongs to a file whose blocks
     * lie inside the file and cover every scanline of the window exactly once */
    const uint64_t n_blocks = ((uint64_t)h + lines_per_block - 1) / lines_per_block;
    if (n_blocks > c.left() / 8) return io_fail(FTN_ERR_INVALID_ARGUMENT, "truncated OpenEXR offset table");
    std::vector<unsigned char> raw, seen((size_t)n_blocks, 0);
    for (uint64_t b = 0; b < n_blocks; b++) {
        uint64_t off; c.u64(&off);
        if (off > buf.size() || buf.size() - off < 8) return io_fail(FTN_ERR_INVALID_ARGUMENT, "truncated OpenEXR scanline");
        Cursor blk{buf.data(), buf.size(), (size_t)off};
        int32_t y, n; const unsigned char* data;
        blk.i32(&y); blk.i32(&n);
        const int64_t rel = (int64_t)y - dw[1];
        if (n < 0 || !blk.bytes((size_t)n, &data) || rel < 0 || rel >= h || (uint64_t)rel % lines_per_block) return io_fail(FTN_ERR_INVALID_ARGUMENT, "corrupt OpenEXR scanline");
        if (seen[(size_t)((uint64_t)rel / lines_per_block)]++) return io_fail(FTN_ERR_INVALID_ARGUMENT, "OpenEXR scanline stored twice (and another one never)");
        const uint64_t lines = std::min<uint64_t>(lines_per_block, (uint64_t)(h - rel));
        const uint64_t raw_bytes = row_bytes * lines;
        const bool packed = compression != 0 && (uint64_t)n < raw_bytes;          /* a block that does not shrink is stored raw */
        if (packed) { if (raw_bytes > ((uint64_t)n + 16) * EXR_MAX_RATIO) return io_fail(FTN_ERR_INVALID_ARGUMENT, "corrupt compressed OpenEXR block"); }
        else if ((uint64_t)n != raw_bytes) return io_fail(FTN_ERR_INVALID_ARGUMENT, "unexpected OpenEXR block size");
        if (!rgb_out) continue;
        if (packed) {
            const bool ok = compression == 1 ? rle_decode(data, (size_t)n, raw, (size_t)raw_bytes) : zip_decode(data, (size_t)n, raw, (size_t)raw_bytes);
            if (!ok) return io_fail(FTN_ERR_INVALID_ARGUMENT, "corrupt compressed OpenEXR block");
            data = raw.data();
        }
        for (uint64_t ly = 0; ly < lines; ly++) {
            float* dst = rgb_out + ((size_t)rel + (size_t)ly) * (size_t)w * 3;
            for (int k = 0; k < 3; k++) {
                const unsigned char* src = data + (size_t)(ly * row_bytes + ch_off[ci[k]]);
                if (chans[ci[k]].type == 2) for (int64_t x = 0; x < w; x++) memcpy(&dst[3 * x + k], src + 4 * x, 4);
                else for (int64_t x = 0; x < w; x++) { uint16_t hv; memcpy(&hv, src + 2 * x, 2); dst[3 * x + k] = half_to_float(hv); }
            }
        }
    }
    /* n_blocks distinct blocks, each on its own multiple of lines_per_block inside the window: every scanline was written once */
    if (w_out) *w_out = (uint32_t)w;
    if (h_out) *h_out = (uint32_t)h;
    return FTN_OK;
}

}  // namespace

extern "C" {

const char* ftn_imageio_last_error(void) { return g_io_err.c_str(); }

/* write_exr (src/imageio/exr.rs:47-87): rgb = 3 floats per pixel, row-major, w*h pixels */
static int exr_write(const char* path, const float* rgb, uint32_t w, uint32_t h) {
    if (!path || !rgb || w == 0 || h == 0) return io_fail(FTN_ERR_INVALID_ARGUMENT, "ftn_exr_write: bad arguments");
    std::vector<unsigned char> hd;
    const unsigned char magic[8] = {0x76, 0x2f, 0x31, 0x01, 2, 0, 0, 0};
    hd.insert(hd.end(), magic, magic + 8);
    std::vector<unsigned char> d;
    for (const char* ch : {"B", "G", "R"}) { put_str(d, ch); put_i32(d, 2 /* FLOAT */); d.push_back(1 /* pLinear */); d.push_back(0); d.push_back(0); d.push_back(0); put_i32(d, 1); put_i32(d, 1); }
    d.push_back(0);
    put_attr(hd, "channels", "chlist", d);
    put_attr(hd, "compression", "compression", {0});
    d.clear(); put_i32(d, 0); put_i32(d, 0); put_i32(d, (int32_t)w - 1); put_i32(d, (int32_t)h - 1);
    put_attr(hd, "dataWindow", "box2i", d);
    put_attr(hd, "displayWindow", "box2i", d);
    put_attr(hd, "lineOrder", "lineOrder", {0});
    d.clear(); put_str(d, "image"); d.pop_back();
    put_attr(hd, "name", "string", d);
    d.clear(); put_f32(d, 1.0f); put_attr(hd, "pixelAspectRatio", "float", d);
    d.clear(); put_f32(d, 0.0f); put_f32(d, 0.0f); put_attr(hd, "screenWindowCenter", "v2f", d);
    d.clear(); put_f32(d, 1.0f); put_attr(hd, "screenWindowWidth", "float", d);
    hd.push_back(0);
    const size_t row_bytes = (size_t)w * 12, block = 8 + row_bytes;
    std::vector<uint64_t> offs(h);
    for (uint32_t y = 0; y < h; y++) offs[y] = hd.size() + (size_t)h * 8 + (size_t)y * block;
    std::vector<float> row((size_t)w * 3);
    File file(fopen(path, "wb")); FILE* f = file.f;
    if (!f) return io_fail(FTN_ERR_INVALID_ARGUMENT, std::string("cannot create ") + path);
    bool ok = fwrite(hd.data(), 1, hd.size(), f) == hd.size() && fwrite(offs.data(), 8, h, f) == h;
    for (uint32_t y = 0; y < h && ok; y++) {
        const float* src = rgb + (size_t)y * w * 3;
        for (uint32_t x = 0; x < w; x++) { row[x] = src[3 * x + 2]; row[w + x] = src[3 * x + 1]; row[2 * (size_t)w + x] = src[3 * x]; }
        const int32_t hdr2[2] = {(int32_t)y, (int32_t)row_bytes};
        ok = fwrite(hdr2, 4, 2, f) == 2 && fwrite(row.data(), 4, row.size(), f) == row.size();
    }
    ok = (file.close() == 0) && ok;
    return ok ? FTN_OK : io_fail(FTN_ERR_INTERNAL, std::string("short write to ") + path);
}
int ftn_exr_write(const char* path, const float* rgb, uint32_t w, uint32_t h) {
    return guarded([&] { return exr_write(path, rgb, w, h); });
}

/* include/fountain_hip_idmatte.h: any number of named FLOAT channels and string attributes (the Cryptomatte layers of idmatte.py) */
static int exr_write_channels(const char* path, int32_t w, int32_t h, int32_t n_channels, const char* const* names, const float* const* planes,
                              int32_t n_attrs, const char* const* attr_names, const char* const* attr_values) {
    if (!path || !names || !planes || w <= 0 || h <= 0 || n_channels <= 0 || n_attrs < 0 || (n_attrs > 0 && (!attr_names || !attr_values)))
        return io_fail(FTN_ERR_INVALID_ARGUMENT, "ftn_exr_write_channels: bad arguments");
    std::vector<int32_t> order((size_t)n_channels);
    for (int32_t c = 0; c < n_channels; c++) {
        if (!names[c] || !planes[c]) return io_fail(FTN_ERR_INVALID_ARGUMENT, "ftn_exr_write_channels: null channel name or plane");
        const size_t len = strnlen(names[c], 256);
        if (len == 0 || len >= 256) return io_fail(FTN_ERR_INVALID_ARGUMENT, "ftn_exr_write_channels: a channel name must have 1 to 255 bytes");
        order[(size_t)c] = c;
    }
    for (int32_t a = 0; a < n_attrs; a++) {
        if (!attr_names[a] || !attr_values[a]) return io_fail(FTN_ERR_INVALID_ARGUMENT, "ftn_exr_write_channels: null attribute");
        const size_t len = strnlen(attr_names[a], 256);
        if (len == 0 || len >= 256) return io_fail(FTN_ERR_INVALID_ARGUMENT, "ftn_exr_write_channels: an attribute name must have 1 to 255 bytes");
        if (strlen(attr_values[a]) > (size_t)0x7fffffff) return io_fail(FTN_ERR_INVALID_ARGUMENT, "ftn_exr_write_channels: attribute value too long");
    }
    /* the channel list and every scanline hold the channels sorted by name (bytewise) */
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return strcmp(names[a], names[b]) < 0; });
    for (int32_t c = 1; c < n_channels; c++)
        if (strcmp(names[order[(size_t)c - 1]], names[order[(size_t)c]]) == 0) return io_fail(FTN_ERR_INVALID_ARGUMENT, std::string("ftn_exr_write_channels: duplicate channel name ") + names[order[(size_t)c]]);
    const size_t row_bytes = (size_t)w * 4 * (size_t)n_channels;
    if (row_bytes > (size_t)0x7fffffff) return io_fail(FTN_ERR_INVALID_ARGUMENT, "ftn_exr_write_channels: a scanline of all channels must stay below 2 GiB");
    std::vector<unsigned char> hd;
    const unsigned char magic[8] = {0x76, 0x2f, 0x31, 0x01, 2, 0, 0, 0};
    hd.insert(hd.end(), magic, magic + 8);
    std::vector<unsigned char> d;
    for (int32_t c : order) { put_str(d, names[c]); put_i32(d, 2 /* FLOAT */); d.push_back(0 /* pLinear */); d.push_back(0); d.push_back(0); d.push_back(0); put_i32(d, 1); put_i32(d, 1); }
    d.push_back(0);
    put_attr(hd, "channels", "chlist", d);
    put_attr(hd, "compression", "compression", {0});
    d.clear(); put_i32(d, 0); put_i32(d, 0); put_i32(d, w - 1); put_i32(d, h - 1);
    put_attr(hd, "dataWindow", "box2i", d);
    put_attr(hd, "displayWindow", "box2i", d);
    put_attr(hd, "lineOrder", "lineOrder", {0});
    d.clear(); put_f32(d, 1.0f); put_attr(hd, "pixelAspectRatio", "float", d);
    d.clear(); put_f32(d, 0.0f); put_f32(d, 0.0f); put_attr(hd, "screenWindowCenter", "v2f", d);
    d.clear(); put_f32(d, 1.0f); put_attr(hd, "screenWindowWidth", "float", d);
    for (int32_t a = 0; a < n_attrs; a++) { d.assign(attr_values[a], attr_values[a] + strlen(attr_values[a])); put_attr(hd, attr_names[a], "string", d); }
    hd.push_back(0);
    const size_t block = 8 + row_bytes;
    std::vector<uint64_t> offs((size_t)h);
    for (int32_t y = 0; y < h; y++) offs[(size_t)y] = hd.size() + (size_t)h * 8 + (size_t)y * block;
    File file(fopen(path, "wb")); FILE* f = file.f;
    if (!f) return io_fail(FTN_ERR_INVALID_ARGUMENT, std::string("cannot create ") + path);
    bool ok = fwrite(hd.data(), 1, hd.size(), f) == hd.size() && fwrite(offs.data(), 8, (size_t)h, f) == (size_t)h;
    for (int32_t y = 0; y < h && ok; y++) {
        const int32_t hdr2[2] = {y, (int32_t)row_bytes};
        ok = fwrite(hdr2, 4, 2, f) == 2;
        for (size_t c = 0; c < order.size() && ok; c++) ok = fwrite(planes[order[c]] + (size_t)y * (size_t)w, 4, (size_t)w, f) == (size_t)w;
    }
    ok = (file.close() == 0) && ok;
    return ok ? FTN_OK : io_fail(FTN_ERR_INTERNAL, std::string("short write to ") + path);
}
int ftn_exr_write_channels(const char* path, int32_t w, int32_t h, int32_t n_channels, const char* const* names, const float* const* planes,
                           int32_t n_attrs, const char* const* attr_names, const char* const* attr_values) {
    return guarded([&] { return exr_write_channels(path, w, h, n_channels, names, planes, n_attrs, attr_names, attr_values); });
}

/* read_exr (src/imageio/exr.rs:11-45): first call with rgb_out == NULL for the size */
int ftn_exr_read(const char* path, uint32_t* w_out, uint32_t* h_out, float* rgb_out) {
    return guarded([&] { return exr_read(path, w_out, h_out, rgb_out); });
}

}  // extern "C"

/* load_mipmap's gamma step: imageio/mod.rs:101-107 with inverse_gamma_correct (:169-175); f32::powf through the deterministic powf
 * (detmath.h), like every other transcendental of this library */
int ftn_image_inverse_gamma(float* texels, size_t n) {
    if (!texels && n) return io_fail(FTN_ERR_INVALID_ARGUMENT, "null texel array");
    for (size_t i = 0; i < n; i++) {
        const float v = texels[i];
        texels[i] = v <= 0.04045f ? v * 1.0f / 12.92f : ftn_det::powf_det((v + 0.055f) * 1.0f / 1.055f, 2.4f);
    }
    return FTN_OK;
}
