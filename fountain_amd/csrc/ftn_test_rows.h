/*
 * ftn_test_rows.h -- what the row hooks share (ftn_test_bsdf, ftn_test_light, ftn_test_interaction, ftn_test_camera, ftn_test_material,
 * ftn_test_texture_eval, ftn_test_math): n rows of floats go up, one kernel runs over them, n rows of floats come back.  Each entry point
 * makes its own refusals first and brings its own launch.  Hidden visibility, as everything in ftn_host_internal.h.
 */
#ifndef FTN_TEST_ROWS_H
#define FTN_TEST_ROWS_H
#include "ftn_host_internal.h"

#pragma GCC visibility push(hidden)

/* blocks of 256 lanes for a grid-stride kernel over n rows */
inline unsigned blocks_for(size_t n) { size_t b = (n + 255) / 256; return (unsigned)(b > 8192 ? 8192 : b); }

/* one input of a row hook: n rows of `width` floats on the host */
struct TestRowsIn { const float* rows; size_t width; };

/* Nothing to do for no rows.  Otherwise: the device (set_device), the inputs uploaded, an output of n rows of width_out floats that starts
 * zeroed, launch(device inputs in the order given, device output) on the null stream, the output copied back into rows_out.  The device
 * buffers are freed on every way out */
template <class Launch> int test_rows(int device, size_t n, std::initializer_list<TestRowsIn> ins, float* rows_out, size_t width_out, Launch launch) {
    if (n == 0) return FTN_OK;
    int rc = set_device(device); if (rc) return rc;
    std::vector<DevBuf<float>> dev(ins.size() + 1);
    struct Release { std::vector<DevBuf<float>>& d; ~Release() { for (auto& b : d) b.release(); } } keep{dev};
    std::vector<const float*> din;
    for (const TestRowsIn& in : ins) { DevBuf<float>& b = dev[din.size()]; if ((rc = b.upload(in.rows, in.width * n))) return rc; din.push_back(b.p); }
    DevBuf<float>& dout = dev.back();
    if ((rc = dout.alloc_zero(width_out * n))) return rc;
    launch(din.data(), dout.p);
    const hipError_t e = hipMemcpy(rows_out, dout.p, width_out * n * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(FTN_ERR_NO_DEVICE, hipGetErrorString(e));
    return FTN_OK;
}

#pragma GCC visibility pop
#endif
