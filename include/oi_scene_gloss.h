/*
 * oi_scene_gloss.h -- glossy environment lighting in a scene of many instances (liboi_hip.so, gfx950): the Phong lobe of
 * include/oi_envgloss.h with a reflection-lobe visibility that knows EVERY instance, so that an instance standing in
 * another's reflection lowers its highlight.
 *
 * An addition to include/oi_scene_light.h (every sampled ray against every instance: chunked, integer-accumulated,
 * byte-stable) and include/oi_envgloss.h (the lobe sampler, the prefiltered maps G_s and their lookup), whose model and
 * limits it borrows: it defines none of its own.  Conventions are oi_scene_light.h's: raw device pointers (where an
 * argument is HOST memory it says so), caller-owned memory, nothing allocated, no scratch, asynchronous launches ordered on
 * `stream`, 0 or a negative oi_status, oi_last_error() for the text, 64-bit indices, every argument checked on the host
 * before any launch, no float atomics; the only device atomics are the compaction's integer counters (one add and one max
 * per workgroup); one thread per ray or pixel.
 *
 * THE SEQUENCE (oi_amd.scene.SceneSurface.lobe_visibility / reflection and SceneTransfer.shade run it), after
 * oi_scene_points and oi_scene_point_pixels:
 *
 *   per chunk [j0, j0 + Sc) of the S samples:
 *     oi_scene_lobe_begin         E occluder elements of Sc * n_vis lobe rays
 *     oi_sdf_mlp_fwd_segments / oi_trace_batch_step_anyhit ...   the batched any-hit march, from bound = live[0]
 *     oi_trace_batch_finish       rays in flight -> OI_TRACE_LIMIT
 *     oi_scene_occlusion_resolve  with L = 1 -> V_spec [S * S]: count / S on the mask, 1 off it, integer counts across chunks
 *   oi_scene_reflect              once: the world-frame reflected view vector of every scene pixel
 *   oi_env_shade_glossy_dirs      per 256 environments: oi_env_shade_glossy on the scene's planes, looked up along that plane
 *
 * The split-sum approximation is oi_envgloss.h's; what a scene adds is that V_spec counts a sample as free only when its ray
 * ended OI_TRACE_MISS in every element (oi_scene_occlusion_resolve's rule).  Light that reaches a point by way of another
 * instance (interreflection) is not modelled: a blocked sample is dark.
 */
#ifndef OI_SCENE_GLOSS_H_
#define OI_SCENE_GLOSS_H_

#include "oi_envgloss.h"
#include "oi_scene_light.h"

#ifdef __cplusplus
extern "C" {
#endif

/* o: oi_scene_occlusion_begin's parameters (include/oi_scene_light.h) with L == 1; its ambient, distance, lights and radius are
 * not read (lights, radius may be NULL).  The lobe adds no struct of its own: rays_o [E][N][3], the primary batch's ray origins
 * (the eyes); vis_index [E][N] (oi_scene_visible), the primary ray of visible slot k of element e; N, the rays per element of
 * the primary batch, W * W; shininess, OI_ENVGLOSS_MIN_SHININESS .. OI_ENVGLOSS_MAX_SHININESS and finite.
 * sb: a batch of E occluder elements with sb->s.N == Sc * n_vis.  Ray jj * n_vis + g of element e' asks whether
 * instance e' blocks sample j = j0 + jj of the reflection lobe of visible point g.  With e = elem[g], slot = g - offset[e],
 * k = e * n_pad + slot and the eye rays_o[e][vis_index[e][slot]]:
 *   n = grad[k] / max(|grad[k]|, 1e-6);  v = (eye - hit_points[k]) / max(|.|, 1e-6);  r = 2 ((n . v) n) - v
 *   (oi_occlusion_lobe_begin's expressions, one __device__ function with it)
 *   d = sample j of S about r for the key pixel[g] and `seed`, by oi_occlusion_lobe_begin's polar law: cos(alpha) =
 *   expf(logf(u1) / (s + 1)), sin(alpha) = sqrt(-expm1f(2 logf(u1) / (s + 1))), in oi_occlusion.h's frame of r (one __device__
 *   function with it)
 * The cases are oi_scene_occlusion_begin's ambient form without a distance limit:
 *   n . d <= 0:  OI_TRACE_BACKFACING in every element, not entered -- the horizon is part of the visibility.
 *   e' == e:     the owner's own ray: origin = point + bias n, direction d, near 0, far = the exit of the unit sphere; entered.
 *   e' != e:     origin = w2b_e' applied to (position[g] + bias normal[g]), direction = w2b_e'[:3,:3] (w2b_e[:3,:3]^T d),
 *                every product rounded; culled against the unit sphere as by oi_scene_begin (OI_TRACE_MISS, not entered),
 *                otherwise near and far at the sphere.
 * Every array of the state, counts[e'][0] and live[0] are written as by oi_scene_occlusion_begin.  N >= 1 and E * N < 2^31;
 * 1 <= n_pad <= N; the other limits are oi_scene_occlusion_begin's. */
int oi_scene_lobe_begin(const oi_trace_batch* sb, const oi_scene_occlusion_params* o, const float* rays_o, const int* vis_index,
                        long long N, float shininess, oi_stream_t stream);

/* reflect [S * S][3], WORLD frame: for an owned scene pixel q with e = owner[q], ray = owner_ray[q], k = e * n_pad +
 * vis_slot[e][ray] and the eye rays_o[e][ray], n, v and r as above in e's box frame and
 *   reflect[q] = w2b_e[:3,:3]^T r, the sums under the default contraction (oi_env_shade_glossy's r_w);
 * three zeros off the mask (owner[q] < 0).  rays_o [E][N][3], hit_points / grad [E][n_pad][3], vis_slot [E][N], w2b [E][16].
 * E, N as for oi_scene_transfer_normal; 1 <= n_pad <= N.  Nothing is traced. */
int oi_scene_reflect(const float* rays_o, const float* hit_points, const float* grad, long long n_pad, const int* owner,
                     const int* owner_ray, const int* vis_slot, const float* w2b, int E, long long N, int scene_S,
                     float* reflect, oi_stream_t stream);

/* oi_env_shade_glossy with the world-frame lookup direction r_w given per pixel, dirs [N][3] (read on the mask only), in
 * place of rays_o / hit_points / grad / w2b.  Everything after r_w is oi_env_shade_glossy's, the same code:
 *   d = R_f^T r_w;  theta = acosf(clamp(d.z, -1, 1)),  phi = atan2f(d.y, d.x), + 2 pi when negative;  the bilinear lookup in
 *   map map_index[f] (HOST memory, checked here);  specular = (k_s spec_vis) lookup;
 *   image = max(shading, 0) albedo + specular (the sum skipped where specular == 0);  bg off the mask, specular 0 there.
 * p, spec_vis [N] or NULL (= 1), glossy [M][3][Hp][Wp], rot [F][9], k_s [3], specular [F][3][N] or NULL: oi_env_shade_glossy's,
 * with its limits.  At least one of p->shading, p->image, specular.  Result f of an F-environment launch is bitwise that of
 * the 1-environment launch of environment f; with k_s == 0, image and shading are byte-equal to oi_env_shade's. */
int oi_env_shade_glossy_dirs(const oi_env_shade_params* p, const float* dirs, const float* spec_vis, const float* glossy, int M,
                             int Hp, int Wp, const int* map_index, const float* rot, const float* k_s, float* specular,
                             oi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OI_SCENE_GLOSS_H_ */
