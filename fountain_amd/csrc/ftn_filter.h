/*
 * ftn_filter.h -- host interface of the reconstruction-filtered film (ftn_filter.hip; C ABI: include/fountain_hip_filter.h) and the
 * one piece of code that decides what a sample adds to a pixel, shared by the gather kernel and its host twin.
 */
#ifndef FTN_FILTER_H
#define FTN_FILTER_H
#include "ftn_wavefront.h"

namespace ftn {

/* the filter as the per-term code reads it: radius, its binary32 reciprocal (FilmTile::inv_filter_radius) and Film::filter_table */
struct FilterTable { float radius[2], inv_radius[2]; float w[256]; };

/* One term of the filtered film (the header's footprint, weight and term rules): does the sample at pd = p_film - 0.5 cover pixel
 * (qx, qy)?  If so acc.rgb += (L * 1.0f) * w, acc.w += w with w = table[iy][ix], whatever w is.  rx, ry, the reciprocals and pd by
 * value; every step is one binary32 operation in the reference's order (film.rs:137-169). */
FTN_HD bool filter_add_term(const float* table, float rx, float ry, float inv_rx, float inv_ry, V2 pd, int qx, int qy, float lr, float lg, float lb,
                            float* ar, float* ag, float* ab, float* aw) {
    const int p0x = f2i_sat(ceilf(pd.x - rx)), p1x = f2i_sat(floorf(pd.x + rx));
    const int p0y = f2i_sat(ceilf(pd.y - ry)), p1y = f2i_sat(floorf(pd.y + ry));
    if (qx < p0x || qx > p1x || qy < p0y || qy > p1y) return false;
    int ix = (int)floorf(fabsf(((float)qx - pd.x) * inv_rx * 16.0f)), iy = (int)floorf(fabsf(((float)qy - pd.y) * inv_ry * 16.0f));
    ix = ix < 15 ? ix : 15; iy = iy < 15 ? iy : 15;
    const float w = table[iy * 16 + ix];
    *ar += (lr * 1.0f) * w; *ag += (lg * 1.0f) * w; *ab += (lb * 1.0f) * w; *aw += w;
    return true;
}

/* How far, in pixels, the sample of source pixel p (p_film in [p, p + 1], both ends reached) can land from p along an axis of radius r,
 * for source pixels in [lo, hi): floor(r + 0.5) in exact arithmetic.  In binary32 pd - r is rounded, and where r + 0.5 lies within
 * half an ulp of the coordinate below an integer the footprint reaches one pixel further; the rounding error grows with the
 * coordinate, so the reach is taken from the film's own end pixels with the per-term code's operations. */
inline int filter_margin(float r, int lo, int hi) {
    int m = f2i_sat(floorf(r + 0.5f));
    const int ends[2] = {lo, hi - 1};
    for (int k = 0; k < 2; k++) {
        const float p = (float)ends[k];
        m = std::max(m, ends[k] - f2i_sat(ceilf((p - 0.5f) - r)));
        m = std::max(m, f2i_sat(floorf((p + 0.5f) + r)) - ends[k]);
    }
    return m;
}

/* An output tile of the gather: a 16 x 16 tile of the sample-bounds grid that meets the crop and has a selected tile in its 3 x 3 ring */
struct FilterOutTile { int gx, gy; };
/* What k_ff_gather needs beside the pass's buffers.  grid_map[gy * grid_w + gx] = index of that grid tile in the call's tile list, or
 * -1; acc = one float4 {r, g, b, weight} per crop pixel, the running sums of the call. */
struct FilterGather {
    FilterTable T;
    int sb[4];                      /* the film's sample bounds (the grid's origin is sb[0], sb[1]) */
    int grid_w, grid_h;
    int mx, my;                     /* the staged window is the output tile grown by this margin */
    uint32_t chunk;                 /* sample indices staged through LDS at a time */
    const int* grid_map; const FilterOutTile* out_tiles; uint32_t n_out_tiles;
    float4* acc;
};
/* LDS bytes of one k_ff_gather workgroup for margins (mx, my) and `chunk` sample indices */
size_t filter_gather_lds(int mx, int my, uint32_t chunk);
/* ftn_render's wavefront passes with k_ff_gather behind every pass.  P as the caller sets it up for the beauty (see
 * ftn_filter_host.cpp: its radius is the box's 0.5); G.acc zeroed by the caller.  Then launch_filter_merge finishes the call. */
int wavefront_filtered(WavefrontState** state, const RenderParams& P, const std::vector<DTile>& tiles, bool count, bool count_production,
                       const FilterGather& G, hipStream_t stream, WavefrontTimes* times);
/* out (ftn_pixel per crop pixel) += {rgb_to_xyz(acc.rgb), acc.w} */
void launch_filter_merge(const RenderParams& P, const float4* acc, float4* out, hipStream_t stream);

}  // namespace ftn
#endif
