/*
 * ftn_bvh_host.h -- what scene construction (ftn_scene_host.cpp) asks of the BVH unit (ftn_bvh_host.cpp): the reference's tree over a set of
 * boxes, and the three record trees the traversal kernels walk, each built from that tree's nodes alone.  The layouts of the records are
 * described where they are built.  Hidden visibility, as everything in ftn_host_internal.h.
 */
#ifndef FTN_BVH_HOST_H
#define FTN_BVH_HOST_H
#include "ftn_host_internal.h"

#pragma GCC visibility push(hidden)

inline Aabb aabb_empty() { Aabb b; for (int i = 0; i < 3; i++) { b.lo[i] = 3.402823466e+38f; b.hi[i] = -3.402823466e+38f; } return b; }
inline void aabb_join_point(Aabb& b, ftn::V3 p) { b.lo[0] = ftn::fmin_(b.lo[0], p.x); b.lo[1] = ftn::fmin_(b.lo[1], p.y); b.lo[2] = ftn::fmin_(b.lo[2], p.z); b.hi[0] = ftn::fmax_(b.hi[0], p.x); b.hi[1] = ftn::fmax_(b.hi[1], p.y); b.hi[2] = ftn::fmax_(b.hi[2], p.z); }

/* BVH::build (bvh.rs:27-158) over the primitives' bounds (at least one): hs->nodes in flattened DFS order, hs->order, hs->max_depth.
 * On host threads from 65536 primitives on, with the serial build's result node for node */
void build_bvh(const std::vector<Aabb>& bounds, HostScene* hs);

/* four-box records (DScene::quad), 32 floats each */
struct QuadBvh { std::vector<float> rec; uint32_t n_records = 0, stack_bound = 0; bool ok = false; };
void build_quads(const std::vector<ftn_bvh_node>& nodes, QuadBvh* out);
/* eight-box occlusion records (DScene::oct), 32 words each, and the exact boxes of the leaves that need one */
struct OctBvh { std::vector<uint32_t> rec; std::vector<float4> xbox; uint32_t n_records = 0, stack_bound = 0; bool ok = false; };
void build_octs(const std::vector<ftn_bvh_node>& nodes, const std::vector<float4>& geom, OctBvh* out);
/* 64-byte four-box records (DScene::quad64), 16 words each, from the 128-byte ones */
struct Quad64Bvh { std::vector<uint32_t> rec; std::vector<float4> xbox; uint32_t n_records = 0, stack_bound = 0; bool ok = false; };
void build_quad64s(const QuadBvh& qb, const std::vector<float4>& geom, Quad64Bvh* out);

#pragma GCC visibility pop
#endif
