/*
 * oi_scene_aa.h -- adaptive anti-aliasing of a scene of many instances (liboi_hip.so, gfx950).
 *
 * An addition to oi_scene.h and oi_aa.h, and their conventions hold: raw device pointers, caller-owned memory, nothing
 * allocated, no scratch, asynchronous launches ordered on `stream`, 0 or a negative oi_status, oi_last_error() for the text,
 * 64-bit indices, every argument checked on the host before any launch, no float atomics; the only device atomics are the
 * integer counters of the compactions (one add and at most one max per workgroup); 256-thread workgroups, one thread per scene
 * pixel or ray, the element index is blockIdx.y where a launch is per element.  The header defines no type of its own.
 *
 * A scene shows two kinds of staircase: the outline of every instance against the background, and the contour along which a
 * nearer instance hides a farther one, where both sides are hits.  The pixels at either get S - 1 more rays through points
 * inside the pixel, one ray PER INSTANCE and sample, which are one more batch of E elements:
 *
 *   oi_scene_aa_classify   which scene pixels need more samples, from the owner map and the visible hits of the primary trace
 *   oi_scene_aa_begin      per instance the sub-pixel rays of the flagged pixels, started as oi_scene_begin starts rays
 *   (the batched march, oi_trace_batch_finish, oi_scene_resolve, oi_scene_visible, oi_trace_batch_gather, the full MLP pass,
 *    the shadow and occlusion begins and resolves, the scene shades: unchanged)
 *   oi_aa_resolve_strided  per plane and scene pixel the centre value or the mean of its S samples
 *
 * THE VIRTUAL IMAGE.  Every entry of oi_scene.h speaks of E windows of W x W rays in an S x S image.  The n_sub = (S - 1) *
 * n_edge sub-samples take that shape: a scene image of Q x Q pixels, Q = ceil(sqrt(n_sub)), in which every instance's window
 * is the whole image (W = S = Q, origin (0, 0)).  Local ray q of every element is virtual pixel q, the sub-sample (j - 1) *
 * n_edge + e' for q < n_sub and padding behind (fewer than 2 Q + 1 rays per element, never traced).  With that shape the
 * scene's resolve, visible lists, points, shadows and shades run on the sub-samples as they run on the scene.
 */
#ifndef OI_SCENE_AA_H_
#define OI_SCENE_AA_H_

#include "oi_aa.h"
#include "oi_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

/* owner, owner_ray [S * S] (oi_scene_resolve), vis_slot [E][N] (oi_scene_visible), hit_points and grad [E][n_pad][3]: the
 * visible points of every instance in its own box frame and the raw SDF gradient there.  N = W * W rays per element.
 * owned(p): 0 <= owner[p] < E, 0 <= owner_ray[p] < N and 0 <= vis_slot[owner[p]][owner_ray[p]] < n_pad; anything else is read as
 * "not owned", so no index leaves the arrays.  Scene pixel p is FLAGGED when one of its up to 8 neighbours q inside the
 * image satisfies one of
 *   (mask)      owned(p) != owned(q)
 *   (instance)  both owned, owner[p] != owner[q]: an occluding contour between two instances, or two instances that touch
 *   (plane), (normal)  both owned by the same instance e: oi_aa_classify's two expressions (oi_aa.h) on e's box-frame points
 *               and raw gradients, one __device__ function with that entry.  The poses are rigid, so lengths and angles in
 *               the box frame are those of the world.
 * 0 <= plane_threshold < 1, 0 <= cos_threshold < 1.  edge_index [S * S], edge_slot [S * S] and count are written exactly as by
 * oi_aa_classify: the first *count entries of edge_index hold the flagged pixels in no fixed order, edge_slot every pixel's
 * position there or -1, count is cleared by a launch ahead of the kernel.
 * 1 <= E <= OI_TRACE_BATCH_MAX_ELEMS, N >= 1, E * N < 2^31, 0 <= n_pad <= N (0: nothing is owned, hit_points and grad may be
 * NULL), 1 <= S <= OI_SCENE_MAX_RESOLUTION. */
int oi_scene_aa_classify(const int* owner, const int* owner_ray, const int* vis_slot, const float* hit_points, const float* grad,
                         int E, long long N, long long n_pad, int S, float plane_threshold, float cos_threshold,
                         int* edge_index, int* edge_slot, int* count, oi_stream_t stream);

/* The sub-pixel rays of n_edge flagged scene pixels in every instance's box frame.  b: E elements of b->s.N >= (Sa - 1) *
 * n_edge rays.  c2b [E][16], kinv [9], window [E][2] int32, W, S: oi_scene_begin's, those of the PRIMARY trace.  edge_index
 * [n_edge]: scene pixels Y * S + X.  offsets [Sa][2] (device memory): the samples' positions in units of the pixel pitch, row
 * 0 is not read.
 * Ray q = (j - 1) * n_edge + e' of element e is sample j (1 .. Sa - 1) of pixel edge_index[e'] = (X, Y): with pitch =
 * (float)S / (float)(S - 1) and (px, py) the pixel coordinates of oi_gen_rays at offset 0,
 *   px_j = px + offsets[j][0] * pitch,  py_j = py + offsets[j][1] * pitch   (the product and the sum each rounded)
 * and the ray through (px_j, py_j) by oi_gen_rays' arithmetic with c2b_e.  It is then treated as oi_scene_begin treats a ray:
 *   e's window does not cover the PIXEL (X, Y) (the primary's rule, whatever the offset: the centre and the sub-samples of
 *       a pixel see the same instances), or edge_index[e'] lies outside the image:  OI_TRACE_MISS, not entered;
 *   the unit sphere's chord (oi_scene_begin's cull) is empty:  OI_TRACE_MISS, not entered;
 *   otherwise OI_TRACE_MARCH, near_ and far_ at the sphere, t = near_, the first sample point, entered compacted within its
 *       element.
 * A ray that is not entered has steps = 0 and t = near_ = far_ = 0.  Rays q >= (Sa - 1) * n_edge are padding: OI_TRACE_MISS,
 * not entered, with pixel (0, 0)'s centre ray.  Every array of the state is written; counts[e][0] = the entered rays, live[0]
 * their maximum, every other word of counts and live 0; points [E][N][3] wholly, the coordinate origin behind an element's
 * entered rays.  With an offset of 0 a ray, its near_ and far_ and its status are oi_scene_begin's for that pixel and element
 * bit for bit (the same __device__ functions, contraction off in both).
 * 2 <= Sa <= OI_AA_MAX_SAMPLES, 1 <= n_edge <= S * S, 1 <= W, 2 <= S <= OI_SCENE_MAX_RESOLUTION. */
int oi_scene_aa_begin(const oi_trace_batch* b, const float* c2b, const float* kinv, const int* window, int W, int S,
                      const int* edge_index, long long n_edge, const float* offsets, int Sa, oi_stream_t stream);

/* oi_aa_resolve with the planes of `sub` sub_stride elements apart: sub [P][sub_stride], of which the first (S - 1) * n_edge
 * of every plane are read.  (S - 1) * n_edge <= sub_stride < 2^31.  One kernel serves both entries, and oi_aa_resolve is this
 * call with sub_stride = (S - 1) * n_edge.  The scene's sub-samples are the pixels of the Q x Q virtual image, whose planes are
 * Q * Q apart.  (Defined beside oi_aa_resolve in aa.hip.) */
int oi_aa_resolve_strided(const float* centre, const float* sub, long long sub_stride, const int* edge_slot, long long N,
                          long long n_edge, int S, int P, float* out, oi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OI_SCENE_AA_H_ */
