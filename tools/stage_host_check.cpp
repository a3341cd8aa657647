/*
 * stage_host_check.cpp -- a stand-alone caller of the image-space stages' host code, for a sanitizer run on a machine without a GPU:
 * every stage's host twin on a 37 x 53 and a 1 x 1 image (the guided filter with and the plain one without var4, temporal with an
 * unaligned previous history), and the refusal paths of the device and host-buffer entries (null, size, overlap, alignment, no device).
 *
 *   make -C fountain_amd/csrc SUFFIX=_asan EXTRA="-Xarch_host -fsanitize=address,undefined"
 *   hipcc -Xarch_host -fsanitize=address,undefined -x c++ -Iinclude tools/stage_host_check.cpp -o stage_host_check \
 *         -Lfountain_amd -lfountain_hip_asan -Wl,-rpath,$PWD/fountain_amd && ./stage_host_check
 *
 * Without a device the host-buffer entries stop at the no-device refusal, so the device buffers' holder itself runs only on a GPU
 * (tests/test_{denoise,denoise_guided,temporal,display,bloom}.py).  Never run it on a GPU machine: sanitizers are for host code.
 */
#include "fountain_hip.h"
#include "fountain_hip_bloom.h"
#include "fountain_hip_denoise.h"
#include "fountain_hip_denoise_guided.h"
#include "fountain_hip_display.h"
#include "fountain_hip_temporal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int failures = 0;
static void expect(int got, int want, const char* what) {
    if (got != want) { printf("FAIL %s: status %d, expected %d (%s)\n", what, got, want, ftn_last_error()); failures++; }
}

static void stages(int w, int h) {
    const size_t n = (size_t)w * (size_t)h;
    std::vector<float> rgb(3 * n), gb(12 * n, 0.5f), var(4 * n, 0.01f), out(3 * n), ovar(4 * n), hist(8 * n), prev(8 * n + 1, 1.0f);
    for (size_t i = 0; i < 3 * n; i++) rgb[i] = 0.01f * (float)(i % 97);
    for (size_t i = 0; i < n; i++) { gb[12 * i + 3] = 0.0f; gb[12 * i + 4] = 0.0f; gb[12 * i + 5] = 1.0f; gb[12 * i + 8] = 2.0f; gb[12 * i + 10] = 1.0f; }

    ftn_denoise_params dp; ftn_denoise_params_default(&dp);
    ftn_denoise_guided_params gp; ftn_denoise_guided_params_default(&gp);
    for (int levels : {0, 1, 5}) {
        dp.levels = gp.levels = levels;
        expect(ftn_denoise_cpu(rgb.data(), gb.data(), w, h, &dp, out.data()), FTN_OK, "ftn_denoise_cpu");
        expect(ftn_denoise_guided_cpu(rgb.data(), gb.data(), var.data(), w, h, &gp, out.data()), FTN_OK, "ftn_denoise_guided_cpu");
    }
    expect(ftn_denoise_cpu(rgb.data(), gb.data(), w, h, &dp, rgb.data()), FTN_OK, "ftn_denoise_cpu in place");
    expect(ftn_denoise(rgb.data(), gb.data(), w, h, &dp, out.data(), -1), FTN_ERR_NO_DEVICE, "ftn_denoise");
    expect(ftn_denoise_guided(rgb.data(), gb.data(), var.data(), w, h, &gp, out.data(), -1), FTN_ERR_NO_DEVICE, "ftn_denoise_guided");
    expect(ftn_denoise_guided_cpu(rgb.data(), gb.data(), nullptr, w, h, &gp, out.data()), FTN_ERR_INVALID_ARGUMENT, "guided, null var4");
    std::vector<float> ws(16 * n + 4);
    expect(ftn_denoise_device(rgb.data(), gb.data(), w, h, &dp, out.data(), ws.data(), nullptr), FTN_ERR_NO_DEVICE, "ftn_denoise_device");
    expect(ftn_denoise_device(rgb.data(), gb.data(), w, h, &dp, rgb.data(), ws.data(), nullptr), FTN_ERR_INVALID_ARGUMENT, "denoise overlap");
    expect(ftn_denoise_guided_device(rgb.data(), gb.data(), var.data(), w, h, &gp, out.data(), var.data(), nullptr), FTN_ERR_INVALID_ARGUMENT,
           "guided workspace overlap");
    expect(ftn_denoise_device(rgb.data(), gb.data(), w, h, &dp, out.data(), ws.data() + 1, nullptr), FTN_ERR_INVALID_ARGUMENT, "denoise misaligned");
    dp.sigma_color = -1.0f;
    expect(ftn_denoise_cpu(rgb.data(), gb.data(), w, h, &dp, out.data()), FTN_ERR_INVALID_ARGUMENT, "denoise sigma");

    ftn_camera_desc cam;
    memset(&cam, 0, sizeof(cam));
    for (int i = 0; i < 4; i++) cam.camera_to_world.m[5 * i] = cam.camera_to_world.inv[5 * i] = cam.raster_to_camera.m[5 * i] = cam.raster_to_camera.inv[5 * i] = 1.0f;
    ftn_film_desc film;
    memset(&film, 0, sizeof(film));
    film.full_resolution[0] = film.crop[2] = w; film.full_resolution[1] = film.crop[3] = h;
    ftn_temporal_params tp; ftn_temporal_params_default(&tp);
    const ftn_temporal_pixel* unaligned = (const ftn_temporal_pixel*)(prev.data() + 1);
    expect(ftn_temporal_accumulate_cpu(rgb.data(), gb.data(), var.data(), &cam, &film, w, h, nullptr, nullptr, nullptr, &tp, (ftn_temporal_pixel*)hist.data(),
                                       out.data(), ovar.data()), FTN_OK, "temporal first frame");
    expect(ftn_temporal_accumulate_cpu(rgb.data(), gb.data(), var.data(), &cam, &film, w, h, &cam, gb.data(), unaligned, &tp, (ftn_temporal_pixel*)hist.data(),
                                       out.data(), ovar.data()), FTN_OK, "temporal second frame");
    expect(ftn_temporal_accumulate(rgb.data(), gb.data(), var.data(), &cam, &film, w, h, &cam, gb.data(), unaligned, &tp, (ftn_temporal_pixel*)hist.data(),
                                   out.data(), ovar.data(), -1), FTN_ERR_NO_DEVICE, "ftn_temporal_accumulate");
    expect(ftn_temporal_accumulate_device(rgb.data(), gb.data(), var.data(), &cam, &film, w, h, nullptr, nullptr, nullptr, &tp, hist.data(), out.data(), out.data(),
                                          nullptr), FTN_ERR_INVALID_ARGUMENT, "temporal outputs overlap");
    expect(ftn_temporal_accumulate_device(rgb.data(), gb.data(), var.data(), &cam, &film, w, h, &cam, gb.data(), nullptr, &tp, hist.data(), out.data(), ovar.data(),
                                          nullptr), FTN_ERR_INVALID_ARGUMENT, "temporal half a previous frame");

    ftn_display_params sp; ftn_display_params_default(&sp);
    std::vector<uint32_t> words(FTN_DISPLAY_HIST_WORDS), codes(n);
    ftn_display_info info;
    expect(ftn_display_histogram_cpu(rgb.data(), w, h, words.data()), FTN_OK, "ftn_display_histogram_cpu");
    sp.flags = FTN_DISPLAY_AUTO_EXPOSURE;
    expect(ftn_display_exposure(words.data(), &sp, &info), FTN_OK, "ftn_display_exposure");
    expect(ftn_display_encode_cpu(rgb.data(), w, h, &sp, info.scale, out.data(), codes.data()), FTN_OK, "ftn_display_encode_cpu");
    expect(ftn_display_encode_cpu(rgb.data(), w, h, &sp, info.scale, nullptr, codes.data()), FTN_OK, "ftn_display_encode_cpu without out_rgb");
    expect(ftn_display(rgb.data(), w, h, &sp, nullptr, codes.data(), &info, -1), FTN_ERR_NO_DEVICE, "ftn_display");
    expect(ftn_display_histogram(rgb.data(), w, h, words.data(), -1), FTN_ERR_NO_DEVICE, "ftn_display_histogram");
    expect(ftn_display_encode_device(rgb.data(), w, h, &sp, 1.0f, nullptr, rgb.data(), nullptr), FTN_ERR_INVALID_ARGUMENT, "display overlap");
    expect(ftn_display_encode(rgb.data(), 0, h, &sp, 1.0f, nullptr, codes.data(), -1), FTN_ERR_INVALID_ARGUMENT, "display w = 0");

    ftn_bloom_params bp; ftn_bloom_params_default(&bp);
    for (int levels : {0, 3, 12}) {
        bp.levels = levels;
        expect(ftn_bloom_cpu(rgb.data(), w, h, &bp, out.data()), FTN_OK, "ftn_bloom_cpu");
    }
    bp.strength = 0.0f;
    expect(ftn_bloom_cpu(rgb.data(), w, h, &bp, out.data()), FTN_OK, "ftn_bloom_cpu, strength 0");
    expect(ftn_bloom(rgb.data(), w, h, &bp, out.data(), -1), FTN_ERR_NO_DEVICE, "ftn_bloom");
    bp.levels = 0;
    expect(ftn_bloom_device(rgb.data(), w, h, &bp, rgb.data(), nullptr, nullptr), FTN_ERR_INVALID_ARGUMENT, "bloom overlap, no workspace");
    expect(ftn_bloom_device(rgb.data(), 65536, 32768, &bp, out.data(), nullptr, nullptr), FTN_ERR_INVALID_ARGUMENT, "bloom 2^31 pixels");
}

int main() {
    if (ftn_device_count() > 0) { printf("this check is for a machine without a GPU\n"); return 2; }
    stages(37, 53);
    stages(1, 1);
    printf(failures ? "%d failures\n" : "stage host check: ok\n", failures);
    return failures ? 1 : 0;
}
