/*
 * fountain_hip_subdiv.h -- extension of the C ABI (fountain_hip.h): Loop subdivision surfaces.  A triangle control mesh is refined `levels`
 * times (every level splits a face into four), its vertices are moved to their limit positions and given limit normals; the result is an
 * ordinary indexed triangle mesh with normals for ftn_scene_create (`Shape "loopsubdiv"` of the PBRT reader, SceneBuilder.shape).
 *
 * The reference began this shape (src/shapes/loop_subdiv.rs) and stops in unimplemented!() after building the level-0 tables, so these
 * functions have no orc_* twin in the CPU oracle; FTN_ABI_VERSION and the other extensions are unchanged and this one carries a version of
 * its own.  This comment is the specification.  Two things the reference's stub does are not followed: its boundary test
 * (`.any(|face| face == start_face)`) is inverted and marks closed fans as boundary, and its weight_one_ring skips the first ring vertex
 * and sums the ring before adding the centre.  Its `regular` flag is not kept either: beta(6) below is exactly 1/16.
 *
 * Notation.  NEXT(i) = (i + 1) % 3, PREV(i) = (i + 2) % 3.  idx[f][k]: face f's k-th vertex.  nb[f][k]: the face across the edge
 * idx[f][k] -> idx[f][NEXT(k)], or -1 at a boundary.  vnum(f, v): the k with idx[f][k] == v.  sf[v]: the vertex's start face.  bd[v]: its
 * boundary flag.  All arithmetic on positions is binary32 in the order written, per component, no operation fused.
 *
 * Level 0 (host, once).  sf[v] is the last face, in face order, that uses v.  nb comes from an edge map keyed by the unordered vertex
 * pair, filled in (face, k) order.  bd[v]: walk f = nb[f][vnum(f, v)] from sf[v] until it is -1 (boundary) or back at sf[v] (interior).
 * The valence n of a vertex is the number of faces around an interior vertex and that number + 1 around a boundary vertex (the length of
 * its ring).  Even (kept) vertices keep their valence at every level and odd (new) ones have 6 or 4, so max(max_valence, 6) of the control
 * mesh bounds every walk at every level: the device loops are bounded by it and raise a flag word (FTN_ERR_INTERNAL) instead of spinning.
 *
 * Ring order of v, r_0 .. r_{n-1}.  Interior: from f = sf[v], emit idx[f][NEXT(vnum(f, v))], then step f = nb[f][vnum(f, v)], until back
 * at sf[v].  Boundary: first step forward (f = nb[f][vnum(f, v)]) until nb is -1 and emit that face's next vertex; then repeatedly emit
 * the face's previous vertex idx[f][PREV(vnum(f, v))] and step f = nb[f][PREV(vnum(f, v))] until -1.
 *
 * One level (V vertices, F faces, E edges -> V + E vertices, 4 F faces).
 *   beta(n) = n == 3 ? 0.1875f : 3.0f / (8.0f * (float)n).
 *   1. Even vertices.  Child v keeps index v and bd, and its start face is 4 sf[v] + vnum(sf[v], v).
 *        interior: p = (1 - (float)n * beta(n)) * P[v], then p = p + beta(n) * P[r_j] for j ascending;
 *        boundary: p = ((1 - 2 * 0.125f) * P[v] + 0.125f * P[r_0]) + 0.125f * P[r_{n-1}].
 *   2. Odd vertices.  Slot (f, k) owns its edge iff nb[f][k] < 0 || f < nb[f][k].  The owner's new index is V + the exclusive prefix count
 *      of owning slots in (f, k) order: the order of first discovery in a serial loop over the faces, found without atomics.  With
 *      a = idx[f][k], b = idx[f][NEXT(k)], g = nb[f][k]:
 *        boundary (g < 0): 0.5f * P[a] + 0.5f * P[b], bd = 1;
 *        interior: ((0.375f * P[a] + 0.375f * P[b]) + 0.125f * P[idx[f][PREV(k)]]) + 0.125f * P[idx[g][PREV(vnum(g, b))]], bd = 0.
 *      Its start face is 4 f + 3.  The owner also records the index for the neighbour's slot (g, vnum(g, b)).
 *   3. Topology, per face f and j in 0..2; the children are 4 f + 0..3 and e_j is the odd vertex of slot (f, j):
 *        nb[4f+3][j] = 4f + NEXT(j);   nb[4f+j][NEXT(j)] = 4f + 3;
 *        nb[4f+j][j] = f2 < 0 ? -1 : 4 f2 + vnum(f2, idx[f][j]) with f2 = nb[f][j];   nb[4f+j][PREV(j)]: the same with f2 = nb[f][PREV(j)];
 *        idx[4f+j][j] = idx[f][j];   idx[4f+j][NEXT(j)] = idx[4f+NEXT(j)][j] = idx[4f+3][j] = e_j.
 *   Counts: F' = 4 F, V' = V + E, E' = 2 E + 3 F, boundary vertices B' = B + (boundary edges), boundary edges double.  They are known on
 *   the host before any launch; nothing is read back from the device between levels.
 *
 * After the last level (levels == 0 included).
 *   Limit positions L, from the unmodified last-level P into a second array:
 *        interior: the even interior rule with gamma(n) = 1.0f / ((float)n + 3.0f / (8.0f * beta(n))) in place of beta(n);
 *        boundary: the even boundary rule with 0.2f in place of 0.125f.
 *   Tangents, from the limit positions of the ring (pi_f = 3.14159265358979323846f, sin and cos are detmath.h's sincosf_det):
 *        interior: S = S + c_j * L[r_j], T = T + s_j * L[r_j], j ascending, from +0, (s_j, c_j) = sincos(((2.0f * pi_f) * (float)j) / (float)n);
 *        boundary: S = L[r_{n-1}] - L[r_0] and
 *          n == 2: T = (L[r_0] + L[r_1]) - 2.0f * L[v];
 *          n == 3: T = L[r_1] - L[v];
 *          n == 4: T = ((((-L[r_0]) + 2.0f * L[r_1]) + 2.0f * L[r_2]) - L[r_3]) - 2.0f * L[v];
 *          else:   theta = pi_f / (float)(n - 1), T = sin(theta) * (L[r_0] + L[r_{n-1}]), then
 *                  T = T + ((2.0f * cos(theta) - 2.0f) * sin((float)k * theta)) * L[r_k] for k = 1 .. n - 2, then T = -T.
 *   Normals: N = cross(T, S) = (T.y S.z - T.z S.y, T.z S.x - T.x S.z, T.x S.y - T.y S.x), len = sqrt((N.x N.x + N.y N.y) + N.z N.z) (IEEE),
 *   N = N / len (IEEE divide, per component).  cross(T, S) is on the side of the faces' own winding, cross(p1 - p0, p2 - p0): a control mesh
 *   rendered flat and its refinement agree about the geometric normal.  A zero or non-finite len is a refusal naming the smallest vertex.
 *
 * Outputs: limit positions (V_L x 3), normals (V_L x 3), indices (F_L x 3), in the space of the input; sizes from ftn_loop_subdivide_info.
 *
 * Limits: levels in 0..FTN_SUBDIV_MAX_LEVELS, n_faces * 4^levels <= 2^26, V_L < 2^31.
 *
 * Refusals: FTN_ERR_INVALID_ARGUMENT with a message in ftn_last_error(), in this order, each reached only when everything before it is in
 * order: (1) null pointers; (2) n_vertices <= 0 or n_faces <= 0; (3) levels outside 0..10; (4) n_faces * 4^levels > 2^26; then the topology,
 * each message naming the smallest offending index: (5) an index >= n_vertices (the face); (6) a face with a repeated vertex (the face);
 * (7) an edge used by more than two faces (the third face, in face order, of such an edge); (8) two faces that cross a shared edge in
 * the same direction -- inconsistent winding, where a Moebius strip ends (the later face); (9) a vertex used by no face; (10) a vertex whose
 * walk reaches fewer faces than use it -- two fans pinched at one point; (11) V_L >= 2^31.  Then the entry that runs on the GPU returns
 * FTN_ERR_NO_DEVICE when there is none.  (12) after the run: a vertex whose normal has zero or non-finite length.
 */
#ifndef FOUNTAIN_HIP_SUBDIV_H
#define FOUNTAIN_HIP_SUBDIV_H

#include "fountain_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FTN_SUBDIV_MAX_LEVELS 10
#define FTN_SUBDIV_MAX_FACES (1u << 26)

typedef struct ftn_subdiv_info {        /* 184 bytes; entry l of an array is level l's count, entries above `levels` are 0                */
    int32_t levels;
    int32_t max_valence;                /* of the control mesh; max(max_valence, 6) bounds every level's                                   */
    uint32_t n_vertices[FTN_SUBDIV_MAX_LEVELS + 1];
    uint32_t n_faces[FTN_SUBDIV_MAX_LEVELS + 1];
    uint32_t n_edges[FTN_SUBDIV_MAX_LEVELS + 1];
    uint32_t n_boundary[FTN_SUBDIV_MAX_LEVELS + 1];     /* boundary vertices                                                              */
} ftn_subdiv_info;

/* validates (refusals 1 to 11) and fills the counts; needs no GPU */
int ftn_loop_subdivide_info(const uint32_t* indices, int32_t n_vertices, int32_t n_faces, int32_t levels, ftn_subdiv_info* info);
/* HOST buffers: P 3 n_vertices floats, indices 3 n_faces; out_P and out_N 3 info.n_vertices[levels] floats, out_indices
 * 3 info.n_faces[levels].  Uploads, runs on GPU `device` (-1 = the current one) and downloads. */
int ftn_loop_subdivide(const float* P, int32_t n_vertices, const uint32_t* indices, int32_t n_faces, int32_t levels, float* out_P, float* out_N,
                       uint32_t* out_indices, int32_t device);
/* the host twin: the same bits, on the host's threads, whatever their number; shares the per-element code with the kernels */
int ftn_loop_subdivide_cpu(const float* P, int32_t n_vertices, const uint32_t* indices, int32_t n_faces, int32_t levels, float* out_P, float* out_N,
                           uint32_t* out_indices);

#define FTN_SUBDIV_ABI_VERSION 1
int ftn_subdiv_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FOUNTAIN_HIP_SUBDIV_H */
