/*
 * oi_scene_bounce.h -- one diffuse interreflection bounce between the instances of a scene (liboi_hip.so, gfx950): the
 * bounce of include/oi_envbounce.h with "the surface" replaced by "the union of the instances", so that a red object beside
 * a white one colours it.
 *
 * An addition to include/oi_scene_light.h (every sampled ray against every instance: chunked, byte-stable) and
 * include/oi_envbounce.h (the estimator, the per-channel bounce transfer [3][9] and oi_env_shade_bounce, which shades a scene's
 * planes as it shades a view), whose limits it borrows: it defines none of its own and no struct.  Conventions are
 * oi_scene.h's: raw device pointers, caller-owned memory, nothing allocated, no scratch, asynchronous launches ordered on
 * `stream`, 0 or a negative oi_status, oi_last_error() for the text, 64-bit indices, 256-thread workgroups, one thread per ray
 * or pixel, every argument checked on the host before any launch, no float atomics; the only device atomics are the
 * compaction's integer counters (one add and one max per workgroup).
 *
 * ESTIMATOR.  g a visible point of the scene, e its owner, q its scene pixel; d_j its S transfer rays, drawn ONCE in e's frame
 * by oi_scene_occlusion_begin (ambient != 0, distance = INFINITY) and moved into every other element: nothing about the rays
 * changes.  The direct transfer T0 is oi_scene_transfer_resolve's, unchanged.  Per colour channel
 *
 *   T1[ch][c] = (1 / S) sum_j [sample j has a winner e* and n_j . d_j < 0] rho_ch(y_j) A_band(c) y_c(n_j in the world frame)
 *   shading[ch] = sum_c T0_c L_c[ch] + sum_c T1[ch][c] L_c[ch]                                     (oi_env_shade_bounce)
 *
 * y_j the hit point in e*'s frame, n_j = g / max(|g|, 1e-6) from the full MLP pass there, rho its albedo, d_j the ray's
 * direction IN e*'s FRAME (element e*'s rays_d), the world normal w2b_e*[:3,:3]^T n_j, A = (1, 2/3, 1/4).
 *
 * THE WINNER OF A SAMPLE.  A sample has NO winner when its ray ended, in ANY element, in a status other than OI_TRACE_MISS or
 * OI_TRACE_HIT (OI_TRACE_LIMIT, START_INSIDE, NONFINITE, BACKFACING): it bounces nothing, and it is not free either, so T0 is
 * untouched.  Otherwise the winner is the element whose ray ended OI_TRACE_HIT with the smallest t; on equal t the LOWEST
 * element index wins (oi_scene_resolve's rule).  Without a HIT in any element the sample is free and T0's.  The poses are
 * rigid and the directions are rotations of one world direction, so t is comparable between the elements (oi_scene.h makes
 * the same argument for the primary rays).
 *
 * APPROXIMATIONS (oi_envbounce.h's).  ONE bounce.  The bounce is DIFFUSE (the Phong lobe of the secondary point is ignored).
 * The secondary point's own occlusion is ignored -- by its own instance and by the others --: that OVER-estimates.  Samples
 * without a winner and winners on a back face (n_j . d_j >= 0) bounce nothing: that UNDER-estimates.  Under a constant
 * environment and a white albedo at the secondary points the shading of a pixel is exactly the environment's value when all S
 * of its samples are free or front-face winners: the furnace, per pixel.
 *
 * THE SEQUENCE (oi_amd.scene.SceneSurface.transfer_bounce runs it), after oi_scene_points and oi_scene_point_pixels:
 *
 *   per chunk [j0, j0 + Sc) of the S samples:
 *     oi_scene_occlusion_begin    E occluder elements of Sc * n_vis rays, as for T0 alone
 *     oi_sdf_mlp_fwd_segments / oi_trace_batch_step ...   the batched march in its CLOSEST-hit form (the set of rays that end
 *                                 OI_TRACE_MISS is the same under both steps, oi_occlusion.h)
 *     oi_trace_batch_finish       rays in flight -> OI_TRACE_LIMIT
 *     oi_scene_transfer_resolve   T0's running sums, unchanged
 *     oi_scene_bounce_nearest     winner [Sc * n_vis]
 *     oi_scene_bounce_visible     per element the dense list of the rays it wins; live[last] = n_pad2, read by the host
 *     oi_trace_batch_gather       the E * n_pad2 secondary points; then the full MLP pass there -> grad2, rgb2 (both skipped
 *                                 with n_pad2 == 0): hits that a nearer instance hides never reach the MLP
 *     oi_scene_bounce_resolve     T1's running sums
 *   oi_env_shade_bounce           per 256 environments, on the scene's planes
 */
#ifndef OI_SCENE_BOUNCE_H_
#define OI_SCENE_BOUNCE_H_

#include "oi_envbounce.h"
#include "oi_scene_light.h"

#ifdef __cplusplus
extern "C" {
#endif

/* winner [Nr]: the element that wins ray q of a finished batch of E elements of Nr rays each, or -1.  status, t [E][Nr]: the
 * state's.  One thread per ray, a fixed-order loop over the elements, the reads coalesced across q:
 *   any status[e][q] other than OI_TRACE_MISS and OI_TRACE_HIT -> -1;
 *   otherwise the e with status[e][q] == OI_TRACE_HIT and the smallest t[e][q], the lowest e on equal t (a later element
 *   replaces the winner only when its t is smaller: a NaN never does); -1 without a HIT.
 * 1 <= E <= OI_TRACE_BATCH_MAX_ELEMS, Nr >= 1, E * Nr < 2^31. */
int oi_scene_bounce_nearest(const uint8_t* status, const float* t, int E, long long Nr, int* winner, oi_stream_t stream);

/* Per element e of the batch sb (E elements of Nr = sb->s.N rays) the dense list of the rays it wins, in the shape of
 * oi_scene_visible: sel_index [E][Nr], of which the first n_sel_e entries of row e are written, in no fixed order: the rays
 * q with winner[q] == e; sel_slot [E][Nr], written wholly: the position of ray q in row e's list, -1 where e does not win it.
 * OVERWRITES the hit words: sb->s.counts[e][OI_TRACE_COUNT_WORDS - 1] = n_sel_e, sb->live[OI_TRACE_COUNT_WORDS - 1] = their
 * maximum n_pad2 (one word for the host to read) -- what oi_trace_batch_gather(sb, sel_index, n_pad2) reads.  Nothing else of
 * the state is read or written. */
int oi_scene_bounce_visible(const oi_trace_batch* sb, const int* winner, int* sel_index, int* sel_slot, oi_stream_t stream);

/* Adds the chunk [j0, j0 + Sc) to the running sums of the bounce transfer, bounce [3][9][scene_S * scene_S], planar: one
 * thread per scene pixel, oi_scene_transfer_resolve's arguments and chunk protocol.  winner [Sc * n_vis] and sel_slot
 * [E][Sc * n_vis] of this chunk; rays_d [E][Sc * n_vis][3], the state's; grad2 / rgb2 [E][n_pad2][3], the gradient and albedo of
 * the full MLP pass at the gathered points; owner, owner_ray [scene_S * scene_S], vis_slot [E][N], offset [E], w2b [E][16] as
 * for oi_scene_transfer_resolve.  For an owned pixel (e = owner[q] >= 0) with g = offset[e] + vis_slot[e][owner_ray[q]], the 27
 * sums are loaded from bounce when j0 > 0 (0 otherwise), then for jj = 0 .. Sc - 1 in this order, ray = jj * n_vis + g:
 *   w = winner[ray], skipped unless 0 <= w < E;  k = sel_slot[w][ray], skipped unless 0 <= k < n_pad2 (checked before the gather);
 *   n = grad2[w][k] / max(|.|, 1e-6), d = rays_d[w][ray]; skipped unless n . d < 0 (a back face);
 *   sum[ch][c] = fmaf(rgb2[w][k][ch], A_band(c) y_c(w2b_w[:3,:3]^T n), sum[ch][c])
 * -- oi_bounce_resolve's per-sample term, one __device__ function with it --; when last != 0 one division by S; stored.  Off
 * the mask (owner[q] < 0) the output is 27 zeros.  No atomics, no LDS, a fixed order: two runs give identical bytes, and so do
 * different chunkings.
 * E, N, S, j0, Sc, n_vis, scene_S: oi_scene_transfer_resolve's, with its limits (E * Sc * n_vis < 2^31);
 * 0 <= n_pad2 <= Sc * n_vis; grad2 and rgb2 may be NULL when n_pad2 == 0, and the chunk then adds nothing. */
int oi_scene_bounce_resolve(const int* winner, const int* sel_slot, const float* rays_d, const float* grad2, const float* rgb2,
                            long long n_pad2, const int* owner, const int* owner_ray, const int* vis_slot, const int* offset,
                            const float* w2b, int E, long long N, int S, int j0, int Sc, long long n_vis, int scene_S, int last,
                            float* bounce, oi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OI_SCENE_BOUNCE_H_ */
