/*
 * ftn_display_host.cpp -- C entry points of include/fountain_hip_display.h: the refusals, the exposure (host only, binary64), the host
 * twins of both kernels, the host-buffer entries and the PNG writer.
 *
 * The per-pixel code is ftn_display.h's, shared with the kernels; error reporting, device selection and the host thread budget are the
 * host library's (ftn_host_internal.h).
 */
#include "ftn_host_internal.h"
#include "ftn_display.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <zlib.h>

using namespace ftn;

namespace {

const char* const kNoDevice = "no HIP device available: the fountain HIP path needs an AMD GPU (there is no CPU fallback)";

int size_check(int32_t w, int32_t h) {
    if (w <= 0 || h <= 0) return fail(FTN_ERR_INVALID_ARGUMENT, "image width and height must be positive");
    if ((int64_t)w * (int64_t)h >= ((int64_t)1 << 31)) return fail(FTN_ERR_INVALID_ARGUMENT, "w * h must be below 2^31 pixels");
    return FTN_OK;
}

bool finite(float v) { return (f2u(v) & 0x7f800000u) != 0x7f800000u; }

/* refusals (3) to (8) of the header */
int params_check(const ftn_display_params* p) {
    if (p->tonemap > FTN_DISPLAY_TONEMAP_HABLE) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown ftn_display_params.tonemap");
    if (p->transfer > FTN_DISPLAY_TRANSFER_LINEAR) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown ftn_display_params.transfer");
    if (p->flags & ~(FTN_DISPLAY_DITHER | FTN_DISPLAY_AUTO_EXPOSURE)) return fail(FTN_ERR_INVALID_ARGUMENT, "unknown ftn_display_params.flags bits");
    if (p->reserved != 0) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_display_params.reserved must be 0");
    if (!finite(p->ev) || !finite(p->key) || !finite(p->white) || !finite(p->gamma))
        return fail(FTN_ERR_INVALID_ARGUMENT, "ev, key, white and gamma of ftn_display_params must be finite");
    if (!(p->key > 0.0f) || !(p->white > 0.0f) || !(p->gamma > 0.0f)) return fail(FTN_ERR_INVALID_ARGUMENT, "key, white and gamma of ftn_display_params must be above 0");
    if (!(p->p_lo >= 0.0f && p->p_lo < p->p_hi && p->p_hi <= 1.0f)) return fail(FTN_ERR_INVALID_ARGUMENT, "the percentiles of ftn_display_params need 0 <= p_lo < p_hi <= 1");
    if (!(p->min_ev <= p->max_ev)) return fail(FTN_ERR_INVALID_ARGUMENT, "ftn_display_params needs min_ev <= max_ev");
    return FTN_OK;
}

int scale_check(float scale) {
    if (!finite(scale) || !(scale >= 0.0f)) return fail(FTN_ERR_INVALID_ARGUMENT, "the scale must be finite and not negative");
    return FTN_OK;
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
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
    int rc = size_check(w, h); if (rc) return rc;
    const size_t n = (size_t)w * (size_t)h;
    if (overlaps(hist, FTN_DISPLAY_HIST_WORDS * sizeof(uint32_t), rgb, 3 * n * sizeof(float))) return fail(FTN_ERR_INVALID_ARGUMENT, "the histogram overlaps the input");
    if ((uintptr_t)rgb % 16 || (uintptr_t)hist % 16) return fail(FTN_ERR_INVALID_ARGUMENT, "misaligned buffer: rgb and the histogram need 16 bytes");
    if (ftn_device_count() <= 0) return fail(FTN_ERR_NO_DEVICE, kNoDevice);
    const hipError_t e = launch_display_histogram((const float*)rgb, (uint32_t)n, (uint32_t*)hist, (hipStream_t)stream);
    if (e != hipSuccess) return fail(FTN_ERR_INTERNAL, std::string("display histogram launch: ") + hipGetErrorString(e));
    return FTN_OK;
}

int ftn_display_histogram(const float* rgb, int32_t w, int32_t h, uint32_t* hist, int32_t device) {
    if (!rgb || !hist) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = size_check(w, h); if (rc) return rc;
    if (ftn_device_count() <= 0) return fail(FTN_ERR_NO_DEVICE, kNoDevice);
    if ((rc = set_device(device))) return rc;
    const size_t n = (size_t)w * (size_t)h;
    DevBuf<float> d_rgb; DevBuf<uint32_t> d_hist;
    struct Release { DevBuf<float>* a; DevBuf<uint32_t>* b; ~Release() { a->release(); b->release(); } } keep{&d_rgb, &d_hist};
    if ((rc = d_rgb.upload(rgb, 3 * n)) || (rc = d_hist.alloc_zero(FTN_DISPLAY_HIST_WORDS))) return rc;
    if ((rc = ftn_display_histogram_device(d_rgb.p, w, h, d_hist.p, nullptr))) return rc;
    HIP_TRY(hipMemcpy(hist, d_hist.p, FTN_DISPLAY_HIST_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return FTN_OK;
}

int ftn_display_histogram_cpu(const float* rgb, int32_t w, int32_t h, uint32_t* hist) {
    if (!rgb || !hist) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc = size_check(w, h); if (rc) return rc;
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
    if ((rc = size_check(w, h)) || (rc = params_check(p)) || (rc = scale_check(scale))) return rc;
    const size_t n = (size_t)w * (size_t)h, n_rgb = 3 * n * sizeof(float), n_8 = n * sizeof(uint32_t);
    if (overlaps(out_rgba8, n_8, rgb, n_rgb) || (out_rgb && (overlaps(out_rgb, n_rgb, rgb, n_rgb) || overlaps(out_rgb, n_rgb, out_rgba8, n_8))))
        return fail(FTN_ERR_INVALID_ARGUMENT, "an output overlaps the input or the other output");
    if ((uintptr_t)rgb % 16 || (uintptr_t)out_rgb % 16 || (uintptr_t)out_rgba8 % 16)
        return fail(FTN_ERR_INVALID_ARGUMENT, "misaligned buffer: rgb, out_rgb and out_rgba8 need 16 bytes");
    if (ftn_device_count() <= 0) return fail(FTN_ERR_NO_DEVICE, kNoDevice);
    const hipError_t e = launch_display_encode((const float*)rgb, (uint32_t)w, (uint32_t)n, disp_make(*p, scale), (float*)out_rgb, (uint32_t*)out_rgba8, (hipStream_t)stream);
    if (e != hipSuccess) return fail(FTN_ERR_INTERNAL, std::string("display encode launch: ") + hipGetErrorString(e));
    return FTN_OK;
}

int ftn_display_encode_cpu(const float* rgb, int32_t w, int32_t h, const ftn_display_params* p, float scale, float* out_rgb, uint32_t* out_rgba8) {
    if (!rgb || !p || !out_rgba8) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc;
    if ((rc = size_check(w, h)) || (rc = params_check(p)) || (rc = scale_check(scale))) return rc;
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
    if (ftn_device_count() <= 0) return fail(FTN_ERR_NO_DEVICE, kNoDevice);
    if ((rc = set_device(device))) return rc;
    const size_t n = (size_t)w * (size_t)h;
    DevBuf<float> d_rgb, d_out; DevBuf<uint32_t> d_8, d_hist;
    struct Release { DevBuf<float>* a; DevBuf<float>* b; DevBuf<uint32_t>* c; DevBuf<uint32_t>* d;
                     ~Release() { a->release(); b->release(); c->release(); d->release(); } } keep{&d_rgb, &d_out, &d_8, &d_hist};
    if ((rc = d_rgb.upload(rgb, 3 * n))) return rc;
    float scale;
    if (scale_in) scale = *scale_in;
    else {
        ftn_display_info info;
        std::vector<uint32_t> hist;
        if (p->flags & FTN_DISPLAY_AUTO_EXPOSURE) {
            hist.resize(FTN_DISPLAY_HIST_WORDS);
            if ((rc = d_hist.alloc_zero(FTN_DISPLAY_HIST_WORDS)) || (rc = ftn_display_histogram_device(d_rgb.p, w, h, d_hist.p, nullptr))) return rc;
            HIP_TRY(hipMemcpy(hist.data(), d_hist.p, FTN_DISPLAY_HIST_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
        if ((rc = ftn_display_exposure(hist.empty() ? nullptr : hist.data(), p, &info))) return rc;
        if (info_out) *info_out = info;
        scale = info.scale;
        if ((rc = scale_check(scale))) return rc;
    }
    if (out_rgb) HIP_TRY(hipMalloc((void**)&d_out.p, 3 * n * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&d_8.p, n * sizeof(uint32_t)));
    if ((rc = ftn_display_encode_device(d_rgb.p, w, h, p, scale, d_out.p, d_8.p, nullptr))) return rc;
    if (out_rgb) HIP_TRY(hipMemcpy(out_rgb, d_out.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_rgba8, d_8.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return FTN_OK;
}

int ftn_display_encode(const float* rgb, int32_t w, int32_t h, const ftn_display_params* p, float scale, float* out_rgb, uint32_t* out_rgba8, int32_t device) {
    if (!rgb || !p || !out_rgba8) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc;
    if ((rc = size_check(w, h)) || (rc = params_check(p)) || (rc = scale_check(scale))) return rc;
    return display_host(rgb, w, h, p, &scale, out_rgb, out_rgba8, nullptr, device);
}

int ftn_display(const float* rgb, int32_t w, int32_t h, const ftn_display_params* p, float* out_rgb, uint32_t* out_rgba8, ftn_display_info* info, int32_t device) {
    if (!rgb || !p || !out_rgba8) return fail(FTN_ERR_INVALID_ARGUMENT, "null argument");
    int rc;
    if ((rc = size_check(w, h)) || (rc = params_check(p))) return rc;
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
