/*
 * oi_occlusion.h -- soft shadows and ambient occlusion for the sphere-traced renderer (liboi_hip.so, gfx950): lights with an
 * angular size, S visibility samples per light and visible point, and an occlusion factor on the ambient term.
 *
 * An addition to include/oi_trace.h, whose conventions hold: raw device pointers, caller-owned buffers, nothing allocated,
 * asynchronous launches ordered on `stream`, arguments checked on the host before any launch, 0 or a negative oi_status,
 * 64-bit indices; the only device atomics are the integer per-workgroup counters of the compaction.  The entries work on an
 * oi_trace_state and end with oi_trace_finish, both as oi_trace.h declares them:
 *
 *   oi_occlusion_light_begin | oi_occlusion_ambient_begin    the secondary rays, compacted, counts[0] = the traced ones
 *   for k = 0 .. max_steps - 1:
 *     oi_sdf_mlp_fwd        (grad == NULL) on the first `bound` compacted points
 *     oi_occlusion_step     the ANY-HIT form of oi_trace_step: the ray ends at the first occluder
 *   oi_trace_finish         rays still in flight -> OI_TRACE_LIMIT
 *   oi_occlusion_resolve    S ray states per light and pixel -> the share that ended OI_TRACE_MISS
 *   oi_surface_shade_ao     oi_surface_shade with an occlusion factor on the ambient term
 *
 * Ray layout.  n_hit visible points, L directions (lights), S samples each: s->N == L * S * n_hit and ray
 * q = (l * S + j) * n_hit + i.  S == 1 is the layout of oi_trace_shadow_begin.
 *
 * Sample numbers of sample j at point i (uint32 arithmetic, wrapping; pix = hit_index[i], the pixel's ray index of the
 * primary trace, so a pixel's samples do not depend on its slot in the hit list):
 *
 *   x  = pix * 0x9E3779B9u + seed;  x ^= x >> 16;  x *= 0x7feb352du;  x ^= x >> 15;  x *= 0x846ca68bu;  x ^= x >> 16
 *   u1 = (j + 0.5f) / S                                      one sample per stratum [j / S, (j + 1) / S)
 *   u2 = float((j * 2654435769u + x) >> 8) * 2^-24           24 bits, in [0, 1)
 *
 * Tangent frame (t1, t2) of a unit axis a (Duff et al. 2017, "Building an orthonormal basis, revisited"; no branch):
 *
 *   sg = copysign(1, a.z);  A = -1 / (sg + a.z);  B = a.x * a.y * A
 *   t1 = (1 + sg * a.x * a.x * A,  sg * B,  -sg * a.x)
 *   t2 = (B,  sg + a.y * a.y * A,  -a.y)
 *
 * Direction of a sample at polar angle alpha about a:  phi = 2 pi u2,
 *   d = sin(alpha) cos(phi) t1 + sin(alpha) sin(phi) t2 + cos(alpha) a
 * (sin(alpha) == 0 gives d = a, bit for bit).
 */
#ifndef OI_OCCLUSION_H_
#define OI_OCCLUSION_H_

#include "oi_trace.h"

#ifdef __cplusplus
extern "C" {
#endif

/* samples per light and point (soft shadows) or per point (ambient occlusion): 1 <= S <= OI_OCCLUSION_MAX_SAMPLES */
#define OI_OCCLUSION_MAX_SAMPLES 256

/* Soft-shadow rays.  hit_points / grad [n_hit][3], hit_index [n_hit] (oi_trace_finish's), lights [L][OI_RELIGHT_LIGHT_FLOATS],
 * radius [L] (device memory): the light's angular radius in radians; a value outside [0, pi/2] is clamped into it by the
 * kernel (NaN -> 0).  w2b [16].  1 <= L <= OI_RELIGHT_MAX_LIGHTS, 1 <= S <= OI_OCCLUSION_MAX_SAMPLES, n_hit >= 1,
 * L * S * n_hit == s->N (< 2^31), bias >= 0 and finite.
 * a = the light's direction in the object frame, formed as oi_trace_shadow_begin forms it.  The samples are uniform in solid
 * angle over the cap: with m = u1 (1 - cos radius), cos(alpha) = 1 - m and sin(alpha) = sqrt(max(0, 1 - cos^2(alpha))),
 * the latter evaluated as sqrt(m (2 - m)) (the same number without the cancellation).  n = g / max(|g|, 1e-6).
 * n . d > 0: origin = point + bias n, direction = d, near = 0, far = the exit of the unit sphere (oi_trace_shadow_begin's rule),
 * status MARCH, entered in the active list.  n . d <= 0: OI_TRACE_BACKFACING, not traced -- per sample, so a cap that dips
 * below the horizon is partly occluded by the surface itself.  counts[0] = the traced rays.  Writes every array
 * oi_trace_shadow_begin writes; with radius == 0 and S == 1 each of them is byte-equal to oi_trace_shadow_begin's. */
int oi_occlusion_light_begin(const oi_trace_state* s, const float* hit_points, const float* grad, const int* hit_index,
                             long long n_hit, const float* lights, const float* radius, int L, int S, const float* w2b,
                             float bias, unsigned seed, oi_stream_t stream);

/* Ambient-occlusion rays: L = 1, a = n, s->N == S * n_hit.  Cosine-weighted hemisphere: cos(alpha) = sqrt(1 - u1),
 * sin(alpha) = sqrt(u1).  far = min(distance, the exit of the unit sphere); distance > 0 and finite.  The rest as above. */
int oi_occlusion_ambient_begin(const oi_trace_state* s, const float* hit_points, const float* grad, const int* hit_index,
                               long long n_hit, int S, float bias, float distance, unsigned seed, oi_stream_t stream);

/* oi_trace_step's arguments.  The MARCH phase is oi_trace_step's (s not finite -> NONFINITE, |s| <= tol -> HIT, a negative
 * first sample -> START_INSIDE, t > far -> MISS); a later negative sample ends the ray as OI_TRACE_HIT at that sample, so no
 * ray is ever in OI_TRACE_REFINE.  Compaction, counters and double buffering are oi_trace_step's.  Whether a ray ends
 * OI_TRACE_MISS is decided as by oi_trace_step: everything a refinement can end in is "occluded". */
int oi_occlusion_step(const oi_trace_state* s, const float* sdf, long long bound, int k, float tol, float omega,
                      oi_stream_t stream);

/* out [L][N] of the N pixels of the primary trace: for a pixel with hit slot i the number of samples j whose ray
 * (l * S + j) * n_hit + i ended OI_TRACE_MISS, divided by S (an integer count, one division: the same bits in any order);
 * 1 for a pixel without a hit.  0 <= n_hit <= N < 2^31, L * S * n_hit < 2^31.  S == 1: oi_trace_visibility's map. */
int oi_occlusion_resolve(const uint8_t* status, const int* hit_slot, long long N, long long n_hit, int L, int S, float* out,
                         oi_stream_t stream);

/* oi_surface_params' fields in its order, then the occlusion factor. */
typedef struct oi_surface_ao_params {
  long long N;
  long long n_hit;
  int L;
  const float* rays_o;
  const float* rays_d;
  const float* t;
  const uint8_t* status;
  const int* hit_slot;
  const float* hit_points;
  const float* grad;
  const float* rgb;
  const float* w2b;
  const float* lights;
  const float* bg;
  const float* visibility;
  float* depth;
  float* position;
  float* normal;
  float* normal_world;
  float* albedo;
  float* mask;
  float* image;            /* [L][3][N] (ao ambient + visibility diffuse) albedo + visibility specular */
  const float* ambient_occlusion; /* [N] in [0, 1] or NULL: multiplies the ambient term; NULL: every output is oi_surface_shade's */
} oi_surface_ao_params;

int oi_surface_shade_ao(const oi_surface_ao_params* p, oi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OI_OCCLUSION_H_ */
