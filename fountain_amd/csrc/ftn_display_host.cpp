/*
 * ftn_display_host.cpp -- C entry points of include/fountain_hip_display.h: the refusals, the exposure (host only, binary64), the host
 * twins of both kernels, the host-buffer entries and the PNG writer.
 *
 * The per-pixel code is ftn_display.h's, shared with the kernels; the refusals' shared parts and the device buffers of the host-buffer
 * entries are the stages' scaffold's (ftn_stage_host.h).
 */
#include "ftn_stage_host.h"
#include "ftn_display.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <zlib.h>

using namespace ftn;

namespace {

/* refusals (3) to (8) of the header */
int params_check(const ftn_display_params* p) {
    if (p->tonemap > FTN_DISPLAY_TONEMAP_HABLE) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown ftn_display_params.tonemap");
    if (p->transfer > FTN_DISPLAY_TRANSFER_LINEAR) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown ftn_display_params.transfer");
    if (p->flags & ~(FTN_DISPLAY_DITHER | FTN_DISPLAY_AUTO_EXPOSURE)) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown ftn_display_params.flags bits");
    if (p->reserved != 0) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_display_params.reserved must be 0");
    if (!is_finite(p->ev) || !is_finite(p->key) || !is_finite(p->white) || !is_finite(p->gamma))
        return fail(FTN_ERR_INVALID_ARGUMENT, "ev, key, white and gamma of ftn_display_params must be finite");
    if (!(p->key > 0.0f) || !(p->white > 0.0f) || !(p->gamma > 0.0f)) return fail(FTN_ERR_INVALID_ARGUMENT, "key, white and gamma of ftn_display_params must be above 0");
    if (!(p->p_lo >= 0.0f && p->p_lo < p->p_hi && p->p_hi <= 1.0f)) return fail(FTN_ERR_INVALID_ARGUMENT, "the percentiles of ftn_display_params need 0 <= p_lo < p_hi <= 1");
    if (!(p->min_ev <= p->max_ev)) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_display_params needs min_ev <= max_ev");
    return FTN_OK;
}

int scale_check(float scale) {
    if (!is_finite(scale) || !(scale >= 0.0f)) return fail(FTN_ERR_INVALID_ARGUMENT, "the scale must be finite and not negative");
    return FTN_OK;
}

void put_be32(std::vector<unsigned char>& v, uint32_t x) { for (int s = 24; s >= 0; s -= 8) v.push_back((unsigned char)(x >> s)); }

/* one PNG chunk: length, type, data, the CRC of type and data */
void put_chunk(std::vector<unsigned char>& file, const char type[5], const unsigned char* data, size_t n) {
    put_be32(file, (uint32_t)n);
    const size_t at = file.size();
    file.insert(file.end(), type, type + 4);
    file.insert(file.end(), data, data + n);
    put_be32(file, (uint32_t)crc32(crc32(0L, Z_NULL, 0), file.data() + at, (uInt)(n + 4)));
}

}  // namespace

extern "C" {

static_assert(sizeof(ftn_display_params) == 48 && sizeof(ftn_display_info) == 32, "ABI");
static_assert(FTN_DISPLAY_HIST_WORDS % 4 == 0 && FTN_DISPLAY_HIST_ABOVE < FTN_DISPLAY_HIST_WORDS, "ABI");
int ftn_display_abi_version(void) { return FTN_DISPLAY_ABI_VERSION; }

void ftn_display_params_default(ftn_display_params* p) {
    if (!p) return;
    p->tonemap = FTN_DISPLAY_TONEMAP_ACES;
    p->transfer = FTN_DISPLAY_TRANSFER_SRGB;
    p->flags = 0;
    p->reserved = 0;
    p->ev = 0.0f;
    p->key = 0.18f;
    p->white = 11.2f;
    p->gamma = 2.2f;
    p->p_lo = 0.10f; p->p_hi = 0.95f;
    p->min_ev = -16.0f; p->max_ev = 16.0f;
}

/* ---- the histogram ---- */

int ftn_display_histogram_device(const void* rgb, int32_t w, int32_t h, void* hist, void* stream) {
    if (!rgb || !hist) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = image_check(w, h); if (rc) return rc;
    const size_t n = (size_t)w * (size_t)h;
    const Range r_rgb = {rgb, 12 * n, 16}, r_hist = {hist, FTN_DISPLAY_HIST_WORDS * sizeof(uint32_t), 16};
    if ((rc = overlap_check({r_hist}, {r_rgb}, "the histogram overlaps the input"))) return rc;
    if ((rc = align_check({r_rgb, r_hist}, "misaligned buffer: rgb and the histogram need 16 bytes"))) return rc;
    if ((rc = need_device())) return rc;
    return launched(launch_display_histogram((const float*)rgb, (uint32_t)n, (uint32_t*)hist, (hipStream_t)stream), "display histogram");
}

int ftn_display_histogram(const float* rgb, int32_t w, int32_t h, uint32_t* hist, int32_t device) {
    if (!rgb || !hist) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = image_check(w, h); if (rc) return rc;
    if ((rc = need_device()) || (rc = set_device(device))) return rc;
    StageBufs bufs;
    float* d_rgb; uint32_t* d_hist;
    if ((rc = bufs.upload(rgb, 3 * (size_t)w * (size_t)h, &d_rgb)) || (rc = bufs.alloc_zero(FTN_DISPLAY_HIST_WORDS, &d_hist))) return rc;
    if ((rc = ftn_display_histogram_device(d_rgb, w, h, d_hist, nullptr))) return rc;
    return bufs.copy_back(hist, d_hist, FTN_DISPLAY_HIST_WORDS);
}

int ftn_display_histogram_cpu(const float* rgb, int32_t w, int32_t h, uint32_t* hist) {
    if (!rgb || !hist) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = image_check(w, h); if (rc) return rc;
    const size_t n = (size_t)w * (size_t)h;
    memset(hist, 0, FTN_DISPLAY_HIST_WORDS * sizeof(uint32_t));
    std::mutex m;
    /* a histogram per block of pixels, added under the lock: integer sums, so the number of blocks changes nothing */
    parallel_for(n, [&](size_t i0, size_t i1) {
        std::vector<uint32_t> local(FTN_DISPLAY_HIST_WORDS, 0u);
        for (size_t i = i0; i < i1; i++) local[disp_bin(disp_luminance(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]))]++;
        std::lock_guard<std::mutex> lock(m);
        for (int k = 0; k < FTN_DISPLAY_HIST_WORDS; k++) hist[k] += local[k];
    });
    return FTN_OK;
}

/* ---- the exposure ---- */

int ftn_display_exposure(const uint32_t* hist, const ftn_display_params* p, ftn_display_info* info) {
    if (!p || !info || (!hist && (p->flags & FTN_DISPLAY_AUTO_EXPOSURE))) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = params_check(p); if (rc) return rc;
    memset(info, 0, sizeof(*info));
    double t = 0.0;
    if (hist) {
        for (int i = 0; i < FTN_DISPLAY_HIST_BINS; i++) t += (double)hist[i];
        info->count_bins = (uint32_t)t;
        info->count_invalid = hist[FTN_DISPLAY_HIST_INVALID]; info->count_below = hist[FTN_DISPLAY_HIST_BELOW]; info->count_above = hist[FTN_DISPLAY_HIST_ABOVE];
    }
    if (!(p->flags & FTN_DISPLAY_AUTO_EXPOSURE)) { info->scale = (float)std::exp2((double)p->ev); return FTN_OK; }
    if (t == 0.0) { info->scale = 1.0f; info->flags = FTN_DISPLAY_INFO_EMPTY; return FTN_OK; }
    const double lo = (double)p->p_lo * t, hi = (double)p->p_hi * t;
    double c = 0.0, sw = 0.0, swr = 0.0;
    for (int i = 0; i < FTN_DISPLAY_HIST_BINS; i++) {
        const double n = (double)hist[i], wgt = std::max(0.0, std::min(c + n, hi) - std::max(c, lo));
        c += n;
        if (wgt > 0.0) {
            const double rep = (double)((i >> 3) - 24) + std::log2(1.0 + ((double)(i & 7) + 0.5) / 8.0);
            sw += wgt; swr += wgt * rep;
        }
    }
    info->avg_log2 = swr / sw;
    const double s = (double)p->key / std::exp2(info->avg_log2);
    info->scale = (float)std::min(std::max(s, std::exp2((double)p->min_ev)), std::exp2((double)p->max_ev));
    return FTN_OK;
}

/* ---- the encode ---- */

int ftn_display_encode_device(const void* rgb, int32_t w, int32_t h, const ftn_display_params* p, float scale, void* out_rgb, void* out_rgba8, void* stream) {
    if (!rgb || !p || !out_rgba8) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc;
    if ((rc = image_check(w, h)) || (rc = params_check(p)) || (rc = scale_check(scale))) return rc;
    const size_t n = (size_t)w * (size_t)h;
    const Range r_rgb = {rgb, 12 * n, 16}, r_out = {out_rgb, 12 * n, 16}, r_8 = {out_rgba8, 4 * n, 16};     /* (out_rgb may be null) */
    if ((rc = overlap_check({r_8, r_out}, {r_rgb}, "an output overlaps the input or the other output"))) return rc;
    if ((rc = align_check({r_rgb, r_out, r_8}, "misaligned buffer: rgb, out_rgb and out_rgba8 need 16 bytes"))) return rc;
    if ((rc = need_device())) return rc;
    return launched(launch_display_encode((const float*)rgb, (uint32_t)w, (uint32_t)n, disp_make(*p, scale), (float*)out_rgb, (uint32_t*)out_rgba8,
                                          (hipStream_t)stream), "display encode");
}

int ftn_display_encode_cpu(const float* rgb, int32_t w, int32_t h, const ftn_display_params* p, float scale, float* out_rgb, uint32_t* out_rgba8) {
    if (!rgb || !p || !out_rgba8) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc;
    if ((rc = image_check(w, h)) || (rc = params_check(p)) || (rc = scale_check(scale))) return rc;
    const DispEncode e = disp_make(*p, scale);
    parallel_for((size_t)w * (size_t)h, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            float o[3];
            out_rgba8[i] = disp_pixel(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], (uint32_t)(i % (size_t)w), (uint32_t)(i / (size_t)w), e, o);
            if (out_rgb) { out_rgb[3 * i] = o[0]; out_rgb[3 * i + 1] = o[1]; out_rgb[3 * i + 2] = o[2]; }
        }
    });
    return FTN_OK;
}

/* the host-buffer entries: rgb uploaded once, the histogram only when `info_out` asks for the automatic exposure */
static int display_host(const float* rgb, int32_t w, int32_t h, const ftn_display_params* p, const float* scale_in, float* out_rgb, uint32_t* out_rgba8,
                        ftn_display_info* info_out, int32_t device) {
    int rc;
    if ((rc = need_device()) || (rc = set_device(device))) return rc;
    const size_t n = (size_t)w * (size_t)h;
    StageBufs bufs;
    float *d_rgb, *d_out; uint32_t *d_8, *d_hist;
    if ((rc = bufs.upload(rgb, 3 * n, &d_rgb))) return rc;
    float scale;
    if (scale_in) scale = *scale_in;
    else {
        ftn_display_info info;
        std::vector<uint32_t> hist;
        if (p->flags & FTN_DISPLAY_AUTO_EXPOSURE) {
            hist.resize(FTN_DISPLAY_HIST_WORDS);
            if ((rc = bufs.alloc_zero(FTN_DISPLAY_HIST_WORDS, &d_hist)) || (rc = ftn_display_histogram_device(d_rgb, w, h, d_hist, nullptr)) ||
                (rc = bufs.copy_back(hist.data(), d_hist, FTN_DISPLAY_HIST_WORDS))) return rc;
        }
        if ((rc = ftn_display_exposure(hist.empty() ? nullptr : hist.data(), p, &info))) return rc;
        if (info_out) *info_out = info;
        scale = info.scale;
        if ((rc = scale_check(scale))) return rc;
    }
    if ((rc = bufs.alloc(out_rgb ? 3 * n : 0, &d_out)) || (rc = bufs.alloc(n, &d_8))) return rc;
    if ((rc = ftn_display_encode_device(d_rgb, w, h, p, scale, d_out, d_8, nullptr))) return rc;
    if ((rc = bufs.copy_back(out_rgb, d_out, 3 * n))) return rc;
    return bufs.copy_back(out_rgba8, d_8, n);
}

int ftn_display_encode(const float* rgb, int32_t w, int32_t h, const ftn_display_params* p, float scale, float* out_rgb, uint32_t* out_rgba8, int32_t device) {
    if (!rgb || !p || !out_rgba8) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc;
    if ((rc = image_check(w, h)) || (rc = params_check(p)) || (rc = scale_check(scale))) return rc;
    return display_host(rgb, w, h, p, &scale, out_rgb, out_rgba8, nullptr, device);
}

int ftn_display(const float* rgb, int32_t w, int32_t h, const ftn_display_params* p, float* out_rgb, uint32_t* out_rgba8, ftn_display_info* info, int32_t device) {
    if (!rgb || !p || !out_rgba8) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc;
    if ((rc = image_check(w, h)) || (rc = params_check(p))) return rc;
    return display_host(rgb, w, h, p, nullptr, out_rgb, out_rgba8, info, device);
}

/* ---- PNG ---- */

int ftn_png_write(const char* path, const uint32_t* rgba8, uint32_t w, uint32_t h, uint32_t flags) {
    if (!path || !rgba8) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    if (w == 0 || h == 0 || (uint64_t)w * (uint64_t)h >= ((uint64_t)1 << 31)) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_png_write: w and h must be above 0 and w * h below 2^31");
    const uint32_t gama = flags >> 8;
    if ((flags & 0xfeu) || ((flags & FTN_PNG_GAMA) ? gama == 0 : gama != 0))
        return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_png_write: unknown flag bits, or a gAMA value that does not go with FTN_PNG_GAMA");
    /* the scanlines: filter type 0, then R, G, B of every pixel */
    const size_t row = 1 + 3 * (size_t)w;
    std::vector<unsigned char> raw(row * (size_t)h);
    for (uint32_t y = 0; y < h; y++) {
        unsigned char* d = raw.data() + row * (size_t)y;
        const uint32_t* s = rgba8 + (size_t)w * (size_t)y;
        *d++ = 0;
        for (uint32_t x = 0; x < w; x++) { const uint32_t v = s[x]; *d++ = (unsigned char)v; *d++ = (unsigned char)(v >> 8); *d++ = (unsigned char)(v >> 16); }
    }
    uLongf zn = compressBound((uLong)raw.size());
    std::vector<unsigned char> z(zn);
    if (compress2(z.data(), &zn, raw.data(), (uLong)raw.size(), 6) != Z_OK || zn > 0x7fffffffu) return fail(FTN_ERR_INTERNAL, "ftn_png_write: the zlib stream does not fit one IDAT chunk");
    std::vector<unsigned char> file = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    std::vector<unsigned char> d;
    put_be32(d, w); put_be32(d, h);
    for (unsigned char b : {8, 2, 0, 0, 0}) d.push_back(b);              /* bit depth, colour type RGB, compression, filter method, no interlace */
    put_chunk(file, "IHDR", d.data(), d.size());
    d.clear();
    if (flags & FTN_PNG_GAMA) { put_be32(d, gama); put_chunk(file, "gAMA", d.data(), d.size()); }
    else { d.push_back(0); put_chunk(file, "sRGB", d.data(), d.size()); }
    put_chunk(file, "IDAT", z.data(), (size_t)zn);
    put_chunk(file, "IEND", nullptr, 0);
    FILE* f = fopen(path, "wb");
    if (!f) return fail(FTN_ERR_INVALID_ARGUMENT, std::string("cannot create ") + path);
    bool ok = fwrite(file.data(), 1, file.size(), f) == file.size();
    ok = (fclose(f) == 0) && ok;
    return ok ? FTN_OK : fail(FTN_ERR_INTERNAL, std::string("short write to ") + path);
}

}  /* extern "C" */
