/*
 * ftn_film.h -- Film::add_sample_to_tile (film.rs:136-172; box filter: every table entry is 1.0) for the kernels that add camera samples
 * to a film: the megakernels (ftn_kernels.hip) and the accumulate kernels of the wavefront passes (through ftn_wf_common.h).  The one
 * place that knows a tile's pixel bounds and how a sample's footprint is clamped to them.
 */
#ifndef FTN_FILM_H
#define FTN_FILM_H
#include "ftn_kernels.h"

namespace ftn {

struct FilmCtx {
    int crop[4]; int tpb[4];     /* FilmTile::pixel_bounds of this tile (get_film_tile, film.rs:95-113) */
    int sb[4];                   /* the tile's sample bounds */
    float radius[2];
};
__device__ inline void make_film_ctx(const RenderParams& P, const DTile& t, FilmCtx* F) {
    for (int i = 0; i < 4; i++) F->crop[i] = P.crop[i];
    F->sb[0] = t.x0; F->sb[1] = t.y0; F->sb[2] = t.x1; F->sb[3] = t.y1;
    F->radius[0] = P.radius[0]; F->radius[1] = P.radius[1];
    int p0x = f2i_sat(ceilf((float)t.x0 - 0.5f - P.radius[0])), p0y = f2i_sat(ceilf((float)t.y0 - 0.5f - P.radius[1]));
    int p1x = f2i_sat(ceilf((float)t.x1 - 0.5f + P.radius[0] + 1.0f)), p1y = f2i_sat(ceilf((float)t.y1 - 0.5f - P.radius[1] + 1.0f));   /* sic: -radius, film.rs:100 */
    F->tpb[0] = max(p0x, P.crop[0]); F->tpb[1] = max(p0y, P.crop[1]); F->tpb[2] = min(p1x, P.crop[2]); F->tpb[3] = min(p1y, P.crop[3]);
}
__device__ inline size_t film_idx(const FilmCtx& F, int x, int y) { return (size_t)(y - F.crop[1]) * (size_t)(F.crop[2] - F.crop[0]) + (size_t)(x - F.crop[0]); }

/* the pixels [x0, x1) x [y0, y1) a sample at p_film adds to: its box-filter footprint inside the tile's pixel bounds (film.rs:141-151) */
struct FilmFootprint { int x0, y0, x1, y1; };
__device__ inline FilmFootprint film_footprint(const FilmCtx& F, V2 p_film) {
    float pdx = p_film.x - 0.5f, pdy = p_film.y - 0.5f;
    int p0x = f2i_sat(ceilf(pdx - F.radius[0])), p0y = f2i_sat(ceilf(pdy - F.radius[1]));
    int p1x = f2i_sat(floorf(pdx + F.radius[0])) + 1, p1y = f2i_sat(floorf(pdy + F.radius[1])) + 1;
    p0x = max(p0x, F.tpb[0]); p0y = max(p0y, F.tpb[1]); p1x = min(p1x, F.tpb[2]); p1y = min(p1y, F.tpb[3]);
    return FilmFootprint{p0x, p0y, p1x, p1y};
}

__device__ inline void atomic_add4(float4* p, Rgb c, float w) {
    float* f = reinterpret_cast<float*>(p);
    atomicAdd(f + 0, c.r); atomicAdd(f + 1, c.g); atomicAdd(f + 2, c.b); atomicAdd(f + 3, w);
}
#define FTN_OWN_SERIAL (-2147483647 - 1)   /* film_add: single-writer tile walk */
#define FTN_OWN_NONE (-2147483647)         /* film_add: lane owns no crop pixel */
/* Adds one sample to the accumulators A (own samples) / B (in-tile spill) / C (cross-tile spill) and returns the number of pixels
 * touched.  own_(x,y): the pixel whose register accumulator `acc` belongs to the caller (indexed sampler); the tile-serial sampler
 * passes own_x = FTN_OWN_SERIAL and the tile's one writer adds in-tile pixels straight into A, in stream order. */
__device__ inline int film_add(const FilmCtx& F, float4* A, float4* B, float4* C, V2 p_film, Rgb L, int own_x, int own_y, float4* acc, uint32_t* bc_writes) {
    const FilmFootprint fp = film_footprint(F, p_film);
    const Rgb contrib = L * 1.0f * 1.0f;                     /* radiance * sample_weight * filter_weight (box: 1.0) */
    int touched = 0;
    for (int y = fp.y0; y < fp.y1; y++)
        for (int x = fp.x0; x < fp.x1; x++) {
            touched++;
            if (x == own_x && y == own_y) { acc->x += contrib.r; acc->y += contrib.g; acc->z += contrib.b; acc->w += 1.0f; continue; }
            const bool in_tile = x >= F.sb[0] && x < F.sb[2] && y >= F.sb[1] && y < F.sb[3];
            const size_t i = film_idx(F, x, y);
            if (in_tile && own_x == FTN_OWN_SERIAL) { float4 v = A[i]; v.x += contrib.r; v.y += contrib.g; v.z += contrib.b; v.w += 1.0f; A[i] = v; }
            else { atomic_add4(in_tile ? &B[i] : &C[i], contrib, 1.0f); (*bc_writes)++; }
        }
    return touched;
}

/* The prologue of an accumulate kernel's thread: pixel slot -> its tile (256 slots each, x = slot & 15, y = (slot >> 4) & 15), its pixel,
 * whether the pixel lies inside the tile (valid) and inside the crop window, its index in the per-crop-pixel accumulators (0 outside
 * the crop) and the tile's film context (set when valid). */
struct FilmSlot { bool valid, in_crop; int px, py; size_t ai; FilmCtx F; };
__device__ inline FilmSlot film_slot(const RenderParams& P, uint32_t n_slots, uint32_t slot) {
    FilmSlot s; s.valid = false; s.in_crop = false; s.px = 0; s.py = 0; s.ai = 0;
    if (slot < n_slots) {
        const DTile tile = P.tiles[slot >> 8];
        s.px = tile.x0 + (int)(slot & 15u); s.py = tile.y0 + (int)((slot >> 4) & 15u);
        if (s.px < tile.x1 && s.py < tile.y1) {
            s.valid = true;
            make_film_ctx(P, tile, &s.F);
            s.in_crop = s.px >= P.crop[0] && s.px < P.crop[2] && s.py >= P.crop[1] && s.py < P.crop[3];
            s.ai = s.in_crop ? film_idx(s.F, s.px, s.py) : 0;
        }
    }
    return s;
}

}  // namespace ftn
#endif
