/*
 * oi_local_light.h -- local lights for the sphere-traced renderer (liboi_hip.so, gfx950): point, spot and sphere lights that
 * stand IN the world of the traced view or scene, with shadow rays that end at the light.
 *
 * An addition to include/oi_occlusion.h (the single view) and include/oi_scene_light.h (scenes of many instances), whose
 * conventions hold: raw device pointers, caller-owned memory, nothing allocated, no scratch, asynchronous launches ordered on
 * `stream`, 0 or a negative oi_status, oi_last_error() for the text, 64-bit indices, every argument checked on the host
 * before any launch, no float atomics; the only device atomics are the compaction's integer counters; one thread per ray or
 * pixel.  This header declares no struct: the entries take plain arguments or the structs of the headers it adds to, with
 * `lights` pointing at local records.  The march and the resolves are unchanged -- oi_occlusion_step /
 * oi_trace_batch_step_anyhit already end a ray as OI_TRACE_MISS at t > far, which is how a ray stops at the light;
 * oi_occlusion_resolve / oi_scene_occlusion_resolve count the rays that ended OI_TRACE_MISS:
 *
 *   oi_local_light_begin | oi_scene_local_light_begin     the shadow rays towards the lights, compacted
 *   ... the any-hit march, oi_trace_finish | oi_trace_batch_finish, the resolve ...
 *   oi_surface_shade_local | oi_scene_shade_local          the G-buffer and the Phong image under local lights
 *
 * THE RECORD.  Lights are [L][OI_LOCAL_LIGHT_FLOATS] floats in device memory, 1 <= L <= OI_RELIGHT_MAX_LIGHTS:
 *
 *   [0..2]   position, WORLD frame            [3]  R >= 0: radius of the emitting sphere (0: a point; NaN / negative -> 0)
 *   [4..6]   ambient RGB                      [7]  d0 > 0: the distance at which the light has its nominal colours
 *   [8..10]  diffuse RGB                      [11] cos_outer: cosine of the cone's outer half-angle; <= -1: no cone
 *   [12..14] specular RGB                     [15] shininess
 *   [16..18] cone axis, WORLD frame, pointing away from the light, not necessarily unit      [19] cos_inner (> cos_outer)
 *
 * Floats 4-6, 8-10 and 12-15 stand where OI_RELIGHT_LIGHT_FLOATS has them.
 *
 * ARITHMETIC (fp32; tests/helpers/local_light_ref.py restates it in fp64).  b2w is rigid, so box-frame distances are the
 * world's.  q = w2b (position, 1): the light in the box frame.  A visible point p has the unit normal n = g / max(|g|, 1e-6)
 * and the unit view vector v = (eye - p) / max(|eye - p|, 1e-6).
 *
 * Shading, per pixel, light and channel c:
 *
 *   u = q - p;  dist2 = u . u;  l = u / max(sqrt(dist2), 1e-6)
 *   att  = d0^2 / max(dist2, max(R, OI_LOCAL_LIGHT_MIN_DISTANCE)^2)
 *   a    = w2b[:3,:3] (axis / |axis|);  c = -(l . a);  tt = clamp((c - cos_outer) / (cos_inner - cos_outer), 0, 1)
 *   spot = tt^2 (3 - 2 tt)            (1 when cos_outer <= -1: the axis is not read)
 *   k    = att spot [visibility]
 *   ph   = the Phong geometry of (n, l, v) as oi_surface_shade forms it: ndl = n . l, al = max(v . r, 0) [ndl > 0]
 *   image_c = (ambient_c [ao] + diffuse_c max(ndl, 0) k) albedo_c + specular_c al^shininess k
 *
 * The ambient term is neither attenuated nor shadowed, as on the directional path.
 *
 * Shadow sample j of S for hit i (pixel pix = hit_index[i]) under light l:
 *
 *   o = p + bias n;  w = q - o;  dc = |w|;  axis = w / dc
 *   dc <= R                      -> the origin is inside the light: OI_TRACE_MISS (lit), not entered, steps 0
 *   sin_max = R / dc;  cos_max = sqrt((1 - sin_max)(1 + sin_max));  (u1, u2) = oi_occlusion.h's sample numbers of (pix, seed, j, S)
 *   m = u1 (1 - cos_max);  ca = 1 - m;  sa = sqrt(max(m (2 - m), 0));  d = oi_occlusion.h's direction at (sa, ca, u2) about axis
 *   n . d <= 0                   -> OI_TRACE_BACKFACING, not traced (per sample)
 *   t_light = dc ca - sqrt(max(R^2 - dc^2 sa^2, 0))     where the ray meets the sphere; R == 0: d == axis bit for bit, t_light = dc
 *   near = 0,  far = min(t_light, the exit of the unit sphere),  OI_TRACE_MARCH, entered
 *
 * The samples are uniform in solid angle over the cone the light's sphere subtends at the origin.  Visibility is the
 * unweighted share of a pixel's samples that reach the light, as for oi_occlusion_light_begin's caps.
 * Ray layout: oi_occlusion_light_begin's, q = (l S + j) n_hit + i.
 */
#ifndef OI_LOCAL_LIGHT_H_
#define OI_LOCAL_LIGHT_H_

#include "oi_occlusion.h"
#include "oi_scene_light.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OI_LOCAL_LIGHT_FLOATS 20
/* the smallest distance the inverse-square law is evaluated at (a point light's intensity is bounded) */
#define OI_LOCAL_LIGHT_MIN_DISTANCE 1e-3f

/* The shadow rays of n_hit visible points towards L local lights, S samples each, as stated above.  hit_points / grad
 * [n_hit][3], hit_index [n_hit] (oi_trace_finish's), lights [L][OI_LOCAL_LIGHT_FLOATS], w2b [16].  s->N == L * S * n_hit
 * (< 2^31), 1 <= L <= OI_RELIGHT_MAX_LIGHTS, 1 <= S <= OI_OCCLUSION_MAX_SAMPLES, n_hit >= 1, bias >= 0 and finite.  Writes every
 * array oi_occlusion_light_begin writes; counts[0] = the entered rays.  A ray that is not entered has near = far = 0; the
 * direction of a ray whose origin is inside the light is three zeros. */
int oi_local_light_begin(const oi_trace_state* s, const float* hit_points, const float* grad, const int* hit_index,
                         long long n_hit, const float* lights, int L, int S, const float* w2b, float bias, unsigned seed,
                         oi_stream_t stream);

/* oi_surface_shade_ao with p->lights pointing at [L][OI_LOCAL_LIGHT_FLOATS] local records.  Every G-buffer output is
 * byte-equal to oi_surface_shade's (the same device code); image [L][3][N] as stated above, bg off the mask.  visibility
 * [L][N] and ambient_occlusion [N] may be NULL.  Result l of an L-light launch is bitwise that of the 1-light launch. */
int oi_surface_shade_local(const oi_surface_ao_params* p, oi_stream_t stream);

/* oi_scene_occlusion_begin's chunked layout and rules with p->lights pointing at [L][OI_LOCAL_LIGHT_FLOATS] local records
 * in the WORLD frame: p->ambient must be 0; p->radius and p->distance are not read (radius may be NULL).  With e = elem[g]
 * the direction d and t_light are drawn ONCE in e's frame as stated above (q = w2b_e (position, 1), the key pixel[g]).
 *   dc <= R:     OI_TRACE_MISS in every element, not entered.
 *   n . d <= 0:  OI_TRACE_BACKFACING in every element, not entered.
 *   e' == e:     the ray stated above; entered.
 *   e' != e:     origin and direction moved into e''s frame as oi_scene_occlusion_begin moves them; culled against the unit
 *                sphere (OI_TRACE_MISS, not entered), then clipped to the light: far = min(far, t_light), and a ray with
 *                near >= t_light is OI_TRACE_MISS, not entered (the rule `distance` has for ambient rays). */
int oi_scene_local_light_begin(const oi_trace_batch* sb, const oi_scene_occlusion_params* p, oi_stream_t stream);

/* oi_scene_shade_ao with p->s.lights pointing at [L][OI_LOCAL_LIGHT_FLOATS] local records in the WORLD frame.  For an owned
 * pixel the image is oi_surface_shade_local's on the owner's slices, bit for bit (one device function); every other output
 * is byte-equal to oi_scene_shade's. */
int oi_scene_shade_local(const oi_scene_shade_ao_params* p, oi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OI_LOCAL_LIGHT_H_ */
