/*
 * oi_ground.h -- a ground plane in the world of a scene of many instances (liboi_hip.so, gfx950): a shadow catcher that
 * receives the instances' shadows and ambient occlusion, blocks their own ambient and directional shadow rays, and yields a
 * shadow matte for compositing the scene over a photograph.
 *
 * An addition to include/oi_scene_light.h and include/oi_local_light.h, whose conventions hold: raw device pointers,
 * caller-owned memory, nothing allocated, no scratch, asynchronous launches ordered on `stream`, 0 or a negative oi_status,
 * oi_last_error() for the text, 64-bit indices, every argument checked on the host before any launch, no float atomics; the
 * only device atomics are the compaction's integer counters (one add per workgroup); the element index is blockIdx.y where
 * a launch is per element; one thread per ray, ground point or scene pixel.  The march (oi_sdf_mlp_fwd_segments /
 * oi_trace_batch_step_anyhit) and oi_trace_batch_finish are unchanged.
 *
 * THE RECORD.  [OI_GROUND_FLOATS] floats in device memory, WORLD frame:
 *
 *   [0..2]  unit normal n                     [3]      h: the plane is n . x = h
 *   [4..6]  albedo RGB in [0, 1]              [7]      extent R_g > 0 (INFINITY allowed): the plane exists where |x - c| <= R_g
 *   [8..10] centre c                          [11]     unused
 *
 * The entries cannot read device memory on the host: oi_amd.scene.Ground refuses a normal that is not unit to 1e-4, a
 * non-finite h or c, an albedo outside [0, 1], and oi_amd.scene.SceneSurface.ground a camera on or below the plane.
 *
 * GEOMETRY.  Scene pixel q = Y * S + X has the world ray (o, d) = make_ray(c2w, kinv, 0, 0, S, X, Y), the function
 * oi_scene_begin calls with c2b_e = w2b_e c2w; d is unit and the poses are rigid, so the ground's ray parameter
 * t_g = (h - n . o) / (n . d) is comparable with every instance's t.  q is a GROUND PIXEL when n . d < -1e-6 (the front face),
 * t_g > 0, the point p = o + t_g d (one fused multiply-add per component, formed by ONE device function that every kernel
 * here calls) lies within the extent, and the pixel has no owner or t_g < t_owner strictly (an equal depth goes to the
 * instance).
 *
 * THE SEQUENCE (oi_amd.scene.SceneSurface.ground / shade run it), after oi_scene_resolve:
 *
 *   oi_ground_begin           ground_t and the compacted list of ground pixels; the host sorts the list ascending
 *   per chunk of samples:
 *     oi_ground_rays_begin    E occluder elements of L * Sc * n_g secondary rays of the ground points
 *     oi_sdf_mlp_fwd_segments / oi_trace_batch_step_anyhit ... , oi_trace_batch_finish
 *     oi_ground_resolve       counts of the samples that missed every instance
 *   per finished chunk of the INSTANCES' rays (oi_scene_occlusion_begin, oi_scene_shadow_begin), before its resolve:
 *     oi_ground_occlude       the plane blocks the owner's ray
 *   oi_ground_shade           the ground into the scene's maps, in place; ground_mask and shadow_matte
 *
 * Local-light rays of the instances are not blocked by the ground (oi_ground_occlude takes ambient and directional chunks).
 */
#ifndef OI_GROUND_H_
#define OI_GROUND_H_

#include "oi_local_light.h"
#include "oi_scene_light.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OI_GROUND_FLOATS 12

/* the modes of oi_ground_rays_begin */
#define OI_GROUND_RAYS_CAP 0        /* caps about directional lights [L][OI_RELIGHT_LIGHT_FLOATS]; radius 0, S 1: the hard ray */
#define OI_GROUND_RAYS_HEMISPHERE 1 /* the cosine hemisphere about n, limited by `distance`; L == 1 */
#define OI_GROUND_RAYS_LOCAL 2      /* aimed at local lights [L][OI_LOCAL_LIGHT_FLOATS], ending there */

/* This header declares no struct: the entries take plain arguments, oi_trace_batch.h's batch and oi_scene_light.h's
 * oi_scene_occlusion_params.  What the entries that need the ground points share: c2w [16] the camera's pose (row-major), kinv
 * [9], S the scene's resolution (1 .. OI_SCENE_MAX_RESOLUTION), ground [OI_GROUND_FLOATS], ground_t [S * S] (oi_ground_begin),
 * ground_index [n_g] the ground pixels in ascending order, 1 <= n_g <= S * S. */

/* One thread per scene pixel.  ground_t [S * S] = t_g on the ground pixels, NaN elsewhere; ground_index [S * S]: its first
 * *count entries are the ground pixels in no fixed order (the caller sorts them); count [1] int32 in device memory.
 * owner, owner_ray [S * S] (oi_scene_resolve), t [E][W * W] the primary batch's ray parameters, window [E][2] the instances'
 * windows (the owner's ray is owner_ray: of the windows only their side W is read): owner NULL means no pixel is owned (a scene
 * without a hit), then owner_ray, t and window may be NULL too.  E * W * W < 2^31. */
int oi_ground_begin(const float* c2w, const float* kinv, int S, const float* ground, const int* owner, const int* owner_ray,
                    const float* t, const int* window, int W, int E, float* ground_t, int* ground_index, int* count,
                    oi_stream_t stream);

/* sb: a batch of E occluder elements with sb->s.N == L * Sc * n_g, oi_scene_occlusion_begin's chunked layout: ray
 * (l * Sc + jj) * n_g + g of element e' asks whether instance e' blocks sample j = j0 + jj of light l from ground point g.
 * p: oi_scene_occlusion_begin's parameters, read as follows -- L, S, j0, Sc, seed, bias, w2b as there; n_vis = n_g; pixel
 * [n_g] = ground_index, the key of a point's sample sequence; ambient != 0 exactly when mode is OI_GROUND_RAYS_HEMISPHERE, and
 * then L == 1 and distance > 0 (INFINITY allowed); lights [L][16] (caps) or [L][20] (local), WORLD frame, not read for the
 * hemisphere; radius [L] read for the caps only; n_pad, hit_points, grad, offset, elem, position and normal are not read (may be
 * 0 / NULL).
 * The direction d (and, for local lights, t_light) is drawn ONCE in the world frame by oi_occlusion.h's sample numbers keyed
 * on the scene pixel ground_index[g], sample j of S and seed: the cap about the light's unit direction, the cosine
 * hemisphere about n, or oi_local_light.h's sample from o = p + bias n towards the light at its world position.
 *   n . d <= 0:      OI_TRACE_BACKFACING in every element, not entered.
 *   local, dc <= R:  OI_TRACE_MISS in every element, not entered (the origin is inside the light: lit).
 *   otherwise, in every element e': origin = w2b_e' applied to (p + bias n), direction = w2b_e'[:3,:3] d; culled against the
 *                    unit sphere as by oi_scene_begin (OI_TRACE_MISS, not entered), otherwise near and far at the sphere; the
 *                    hemisphere clips to `distance` and local lights to t_light exactly as oi_scene_occlusion_begin and
 *                    oi_scene_local_light_begin clip: far = min(far, limit), and a ray with near >= limit is OI_TRACE_MISS, not
 *                    entered.
 * Every array of the state, counts[e'][0] and live[0] are written as by oi_scene_shadow_begin. */
int oi_ground_rays_begin(const oi_trace_batch* sb, const oi_scene_occlusion_params* p, int mode, const float* c2w,
                         const float* kinv, int scene_S, const float* ground, const float* ground_t, oi_stream_t stream);

/* count [L][n_g] int32 (the caller's accumulator; overwritten when j0 == 0, added to otherwise), out [L][n_g].  status
 * [E][L * Sc * n_g]: the finished states of the chunk [j0, j0 + Sc).  The count grows by the number of the chunk's samples
 * whose ray ended OI_TRACE_MISS in EVERY element (a fixed-order loop over the elements); with last != 0 out = count / S; out
 * is not touched with last == 0.  oi_scene_occlusion_resolve's rule: a split trace equals the unsplit one byte for byte. */
int oi_ground_resolve(const uint8_t* status, int E, long long n_g, int L, int S, int j0, int Sc, int last, int* count,
                      float* out, oi_stream_t stream);

/* One thread per ground point.  lights: [L][OI_RELIGHT_LIGHT_FLOATS] directional records, or with local != 0
 * [L][OI_LOCAL_LIGHT_FLOATS] local records, WORLD frame, 1 <= L <= OI_RELIGHT_MAX_LIGHTS with image or shadow_matte (otherwise
 * not read); visibility [L][n_g] or NULL; ambient_occlusion [n_g] or NULL.
 * The scene's maps, written IN PLACE at pixel ground_index[g] only, each may be NULL: image [L][3][S * S]; depth [S * S] = t_g;
 * position [S * S][3] = p; normal_world [S * S][3] = n; albedo [S * S][3]; mask [S * S] = 0 (the instances' mask); instance
 * [S * S] = -1.  The ground's own maps, which the caller initialises (0 and 1), each may be NULL: ground_mask [S * S] = 1;
 * shadow_matte [L][3][S * S].
 * Per light l and channel c, with n . l of the light's unit direction (directional) or of l = (q - p) / max(|q - p|, 1e-6)
 * (local), k = visibility (directional) or att spot visibility (local; l, att and spot as oi_scene_shade_local forms them: one
 * device function), ao = ambient_occlusion:
 *   image_c = (ambient_c ao + diffuse_c max(n . l, 0) k) albedo_c          (no specular term)
 *   shadow_matte_c = image_c / (the same expression with ao = 1 and visibility = 1), 1 where that denominator is 0
 * Result l of an L-light launch is bitwise that of the 1-light launch. */
int oi_ground_shade(const float* c2w, const float* kinv, int S, const float* ground, const float* ground_t,
                    const int* ground_index, long long n_g, const float* lights, int L, int local, const float* visibility,
                    const float* ambient_occlusion, float* image, float* depth, float* position, float* normal_world,
                    float* albedo, float* mask, int* instance, float* ground_mask, float* shadow_matte, oi_stream_t stream);

/* The ground as occluder of the instances' rays.  sb: a FINISHED chunk of oi_scene_occlusion_begin or oi_scene_shadow_begin
 * (the same layout with Sc == 1), sb->s.N a multiple of n_vis, before its resolve.  For ray q of point g = q mod n_vis, in
 * the row of the owner e = elem[g] only: the ray is taken to the world frame with b2w_e [E][16]; its status becomes
 * OI_TRACE_HIT when it is OI_TRACE_MISS and the ray meets the plane, either face, within the extent, at 0 < t < limit (limit
 * > 0: `distance` for ambient rays, INFINITY for directional ones).  Nothing else is touched. */
int oi_ground_occlude(const oi_trace_batch* sb, const float* ground, const int* elem, const float* b2w, long long n_vis,
                      float limit, oi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OI_GROUND_H_ */
