/*
 * oi_mesh_attr.h -- intrinsic mesh export: on-surface vertices, normals and albedo (liboi_hip.so, gfx950).
 *
 * Not a reference replacement: the reference's extract_geometry (src/third_party/neus/models/renderer.py:33-41) stops at
 * positions and triangles, so these entries live outside include/oi_hip.h, whose entries each cite the reference interface
 * they replace (as include/oi_relight.h does).  Conventions are oi_hip.h's: raw device pointers, caller-owned buffers,
 * asynchronous launches ordered on `stream`, 0 or a negative oi_status, oi_last_error() for the text.  Nothing is
 * allocated and there is no scratch: every kernel is one thread per vertex over caller-provided arrays.
 *
 * The vertex pass of a marching-cubes mesh (oi_mc_emit) of a field sampled by oi_sdf_lattice, V vertices:
 *
 *   oi_mesh_vertex_world     index-space vertices -> world points through the lattice's own axis arrays
 *   repeat `refine` times:   oi_sdf_mlp_fwd at the points (sdf, d sdf/dx; the albedo of these passes is discarded)
 *                            oi_mesh_newton        p <- p - s g / max(|g|^2, eps), s = sdf + threshold, with safeguards
 *   oi_sdf_mlp_fwd           sdf, d sdf/dx and albedo at the final points
 *   oi_mesh_attr_finalize    unit normals, albedo, the last residual, optionally the interleaved PLY record
 *
 * The MLP passes are the library's full forward, unchanged (include/oi_hip.h: one batch element, n = V points read from
 * memory, the caller's scratch, the pack's own precision); the caller sequences the chain (oi_amd.mesh.vertex_attributes).
 * The mesh is u = -sdf at `threshold`, so the surface the vertices are moved to is sdf = -threshold.  d sdf/dx points to
 * the outside: the side the triangle winding of oi_mc_emit faces ((v1 - v0) x (v2 - v0) towards lower u).
 * No atomics, fixed order: two identical calls give identical bytes.  0 <= V < 2^31; V == 0 launches nothing.
 */
#ifndef OI_MESH_ATTR_H_
#define OI_MESH_ATTR_H_

#include "oi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bits of the per-vertex flag byte (sticky over the steps of one pass) */
#define OI_MESH_FLAG_NONFINITE 1      /* sdf or gradient inf / NaN at the vertex */
#define OI_MESH_FLAG_SMALL_GRADIENT 2 /* |g|^2 < OI_MESH_GRAD_EPS */
#define OI_MESH_FLAG_LIMIT 4          /* the step would leave the half-cell box around the marching-cubes position */
#define OI_MESH_GRAD_EPS 1e-12f
/* Newton steps per pass that callers may ask for (oi_amd.mesh.vertex_attributes checks it) */
#define OI_MESH_MAX_REFINE 8
/* bytes of one interleaved vertex record: x y z nx ny nz (float32, little endian), r g b (uint8); packed, no padding */
#define OI_MESH_RECORD_BYTES 27

/* Index space -> world.  verts_index [V][3] as oi_mc_emit writes them: a vertex lies on one lattice edge, so two of its
 * coordinates are integers and the third is i + t.  Per axis: i = floor(c) clamped to 0 .. n - 1, t = c - i;
 * world = x[i] when t == 0 (x[i + 1] is then not read: i = n - 1 is legal), else fma(t, x[i + 1] - x[i], x[i]) in fp32.
 * xs [nx], ys [ny], zs [nz]: the axis arrays oi_sdf_lattice took, so a vertex with t == 0 is bit-equal to the lattice
 * point the field was evaluated at.  pos [V][3] is written; flags [V] (optional) is cleared: the start of a pass. */
int oi_mesh_vertex_world(const float* verts_index, long long V, const float* xs, const float* ys, const float* zs, int nx,
                         int ny, int nz, float* pos, uint8_t* flags, oi_stream_t stream);

/* One projection step from the (sdf, grad) the MLP pass just wrote at pos.  s = sdf + threshold.
 *   residual [V] (optional) = |s| / |g| BEFORE the step (inf / NaN where the vertex is flagged for it)
 *   pos [V][3] is updated in place to p - s g / max(|g|^2, OI_MESH_GRAD_EPS), unless
 *     - s or g is not finite                      -> OI_MESH_FLAG_NONFINITE
 *     - |g|^2 < OI_MESH_GRAD_EPS                  -> OI_MESH_FLAG_SMALL_GRADIENT
 *     - |new - pos0| > limit on some axis         -> OI_MESH_FLAG_LIMIT
 *   in which cases the vertex keeps its position and the bit is OR-ed into flags [V] (read and written: clear it first,
 *   oi_mesh_vertex_world does).  pos0 [V][3]: the marching-cubes positions; limit_x/y/z: half the lattice spacing per
 *   axis, so a vertex never leaves the cells its triangles were built in. */
int oi_mesh_newton(float* pos, const float* pos0, const float* sdf, const float* grad, long long V, float threshold,
                   float limit_x, float limit_y, float limit_z, float* residual, uint8_t* flags, oi_stream_t stream);

/* After the last MLP pass.  normals [V][3] = g / max(|g|, 1e-6) (the normal of oi_relight_fwd); albedo [V][3] = rgb (the
 * colour head's output, fp32); residual [V] (optional) = |sdf + threshold| / |g|; record (optional, 4-byte aligned,
 * V * OI_MESH_RECORD_BYTES bytes) = pos, normal, round-to-nearest-even of clamp(rgb, 0, 1) * 255 per vertex (NaN -> 0). */
int oi_mesh_attr_finalize(const float* pos, const float* sdf, const float* grad, const float* rgb, long long V,
                          float threshold, float* normals, float* albedo, float* residual, void* record,
                          oi_stream_t stream);

/* The record alone from caller-supplied normals and colours (vertex colours other than the albedo, e.g. shaded ones). */
int oi_mesh_vertex_record(const float* pos, const float* normals, const float* rgb, long long V, void* record,
                          oi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OI_MESH_ATTR_H_ */
